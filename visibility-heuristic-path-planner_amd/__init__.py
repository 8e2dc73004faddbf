"""visibility-heuristic-path-planner_amd -- MI355X-native visibility sweep + visibility-heuristic planner.

Python is plumbing only: this module binds the C ABI of include/vhp.h (libvhp_hip.so, HIP
kernels for gfx950) with ctypes so tests, bench.py and the torch.distributed sharding helper
can drive it.  There is no CPU implementation behind these calls: if the library or a HIP
device is missing they raise.

The directory name is not a Python identifier; import it through the `vhp_amd` shim at the
repo root (``import vhp_amd``) or ``importlib.import_module("visibility-heuristic-path-planner_amd")``.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VHP_LIB") or os.path.join(_HERE, "libvhp_hip.so")  # VHP_LIB: experiment builds
CSRC = os.path.join(_HERE, "csrc")

VHP_OK = 0
VHP_ERR_ARG = 1
VHP_ERR_SOURCE_OOB = 2
VHP_ERR_NOTHING_LIT = 3
VHP_ERR_START_OOB = 10
VHP_ERR_END_OOB = 11
VHP_ERR_START_OCCUPIED = 12
VHP_ERR_END_OCCUPIED = 13
VHP_ERR_MAX_ITER = 20
VHP_ERR_HIP = 100
VHP_ERR_NO_MAP = 101
VHP_ERR_TOO_LARGE = 102
SWEEP_FULL, SWEEP_QUEUE = 0, 1
F64, F32 = 0, 1
U8 = 2   # one byte per cell: the ray-cast calls only
_DTYPES = {F64: np.float64, F32: np.float32, U8: np.uint8}
UNLABELLED = 1000000000000000
SOLVE_PLAIN, SOLVE_BATCH, SOLVE_MAPS_BATCH = 0, 1, 2   # vhp_solve_kind: whose tree the length-field and goal-path calls read
_SOLVE_KINDS = {"plain": SOLVE_PLAIN, "batch": SOLVE_BATCH, "maps": SOLVE_MAPS_BATCH}

# every symbol include/vhp.h declares (tests check the library exports exactly these)
ABI_SYMBOLS = (
    "vhp_create", "vhp_destroy", "vhp_last_error", "vhp_set_stream", "vhp_set_map", "vhp_set_map_device",
    "vhp_sweep_batch", "vhp_sweep_batch_device", "vhp_sync", "vhp_planner_solve", "vhp_reconstruct_path",
    "vhp_raycast_all", "vhp_timing", "vhp_timing_collect", "vhp_set_option", "vhp_sweep_batch_variant", "vhp_planner_solve_variant",
    "vhp_planner_solve_device", "vhp_planner_results_device", "vhp_last_sweep_kernel",
    "vhp_last_elapsed_ms", "vhp_version", "vhp_sweep_batch_offset", "vhp_planner_solve_speculative", "vhp_probe_stores", "vhp_alloc_output", "vhp_alloc_output_cost", "vhp_free_output",
    "vhp_multi_create", "vhp_multi_destroy", "vhp_multi_last_error", "vhp_multi_devices", "vhp_multi_context", "vhp_multi_shard_bounds",
    "vhp_multi_set_map", "vhp_multi_sweep_batch", "vhp_multi_allgather_fields", "vhp_multi_allgather_plan", "vhp_multi_use_rccl",
    "vhp_union_fields_device", "vhp_union_partials_device", "vhp_multi_union_fields",
    "vhp_planner_solve_batch", "vhp_planner_batch_results_device", "vhp_planner_batch_results", "vhp_planner_batch_group",
    "vhp_set_maps", "vhp_set_maps_device", "vhp_sweep_maps_batch", "vhp_sweep_maps_batch_device",
    "vhp_planner_solve_maps_batch", "vhp_planner_maps_batch_results_device", "vhp_planner_maps_batch_results", "vhp_planner_maps_batch_group",
    "vhp_planner_batch_paths", "vhp_planner_batch_paths_device", "vhp_planner_maps_batch_paths", "vhp_planner_maps_batch_paths_device",
    "vhp_planner_path", "vhp_planner_path_device",
    "vhp_planner_length_fields", "vhp_planner_length_fields_device", "vhp_planner_goal_paths", "vhp_planner_goal_paths_device",
    "vhp_raycast_batch", "vhp_raycast_batch_device", "vhp_raycast_maps_batch", "vhp_raycast_maps_batch_device",
    "vhp_line_of_sight", "vhp_line_of_sight_device",
    "vhp_set_maps_windows", "vhp_set_maps_windows_device", "vhp_maps_occupancy", "vhp_maps_occupancy_device",
    "vhp_inflate_map", "vhp_inflate_maps", "vhp_map_occupancy", "vhp_map_occupancy_device",
    "vhp_map_clearance", "vhp_map_clearance_device", "vhp_maps_clearance", "vhp_maps_clearance_device",
)

FOOT_DISC, FOOT_SQUARE, FOOT_DIAMOND = 0, 1, 2   # vhp_footprint
MAX_INFLATE = 64        # VHP_MAX_INFLATE: the largest reach of a footprint, in cells
INFLATE_BORDER = 1      # VHP_INFLATE_BORDER: cells outside the grid count as blocked
CLEARANCE_FAR = 0xFFFF  # VHP_CLEARANCE_FAR: a clearance field's value where no blocked cell lies within p_max
_FOOT_SHAPES = {"disc": FOOT_DISC, "square": FOOT_SQUARE, "diamond": FOOT_DIAMOND}


def footprint(radius=None, shape="disc", p=None):
    """(shape, p) of vhp_inflate_map from a footprint given the Python way: shape "disc", "square" or "diamond" and exactly one of
    `radius` (in cells) and `p` (the C ABI's parameter).  A disc's p is its squared radius, floor(radius^2) computed exactly from the
    value given (an int, a float -- every float is a ratio of integers --, a Fraction or a Decimal), so a fractional radius picks the
    digital disc it means: 2.9 -> 8, 3 -> 9.  The other shapes take an integer radius, which is their p.  ValueError for anything
    else; the reach itself (at most MAX_INFLATE) is the library's to check."""
    from fractions import Fraction
    if shape not in _FOOT_SHAPES:
        raise ValueError("footprint: shape must be one of %s, got %r" % (", ".join(sorted(_FOOT_SHAPES)), shape))
    if (radius is None) == (p is None):
        raise ValueError("footprint: give exactly one of radius and p")
    if p is not None:
        if isinstance(p, bool) or int(p) != p or not 0 <= p < 2 ** 31:
            raise ValueError("footprint: p must be an integer >= 0 (and a C int), got %r" % (p,))
        return _FOOT_SHAPES[shape], int(p)
    try:
        r = Fraction(radius)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("footprint: radius must be a finite number, got %r" % (radius,)) from None
    if r < 0:
        raise ValueError("footprint: radius must be >= 0, got %r" % (radius,))
    if r > 2 ** 15:   # (far past MAX_INFLATE; keeps p inside a C int)
        raise ValueError("footprint: radius %r is beyond any footprint" % (radius,))
    if shape == "disc":
        r2 = r * r
        return FOOT_DISC, r2.numerator // r2.denominator
    if r.denominator != 1:
        raise ValueError("footprint: a %s takes an integer radius, got %r" % (shape, radius))
    return _FOOT_SHAPES[shape], int(r)


class VhpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("vhp status %d: %s" % (code, msg))
        self.code = code


def build_library(force=False):
    """Compile libvhp_hip.so in-tree with hipcc (cross-compiles gfx950 without a GPU)."""
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    return LIB_PATH


_lib = None


def load_library():
    """dlopen libvhp_hip.so.  Import torch first if you use it: both then share one HIP runtime."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libvhp_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C %s`" % CSRC)
    lib = C.CDLL(LIB_PATH)
    vp, i32, u32, u64, f64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_double
    lib.vhp_create.argtypes = [i32, C.POINTER(vp)]
    lib.vhp_destroy.argtypes = [vp]
    lib.vhp_last_error.argtypes = [vp]
    lib.vhp_last_error.restype = C.c_char_p
    lib.vhp_set_stream.argtypes = [vp, vp]
    lib.vhp_set_map.argtypes = [vp, vp, i32, i32]
    lib.vhp_set_map_device.argtypes = [vp, vp, i32, i32]
    lib.vhp_sweep_batch.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.vhp_sweep_batch_device.argtypes = [vp, vp, i32, i32, i32, vp]
    lib.vhp_sync.argtypes = [vp]
    lib.vhp_set_maps.argtypes = [vp, vp, i32, i32, i32]
    lib.vhp_set_maps_device.argtypes = [vp, vp, i32, i32, i32]
    lib.vhp_set_maps_windows.argtypes = [vp, vp, i32, i32, i32]
    lib.vhp_set_maps_windows_device.argtypes = [vp, vp, i32, i32, i32]
    lib.vhp_maps_occupancy.argtypes = [vp, i32, i32, vp]
    lib.vhp_maps_occupancy_device.argtypes = [vp, i32, i32, vp]
    lib.vhp_inflate_map.argtypes = [vp, i32, i32, i32]
    lib.vhp_inflate_maps.argtypes = [vp, i32, i32, i32, i32, i32]
    lib.vhp_map_occupancy.argtypes = [vp, vp]
    lib.vhp_map_occupancy_device.argtypes = [vp, vp]
    lib.vhp_map_clearance.argtypes = [vp, i32, i32, i32, vp]
    lib.vhp_map_clearance_device.argtypes = [vp, i32, i32, i32, vp]
    lib.vhp_maps_clearance.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    lib.vhp_maps_clearance_device.argtypes = [vp, i32, i32, i32, i32, i32, vp]
    lib.vhp_sweep_maps_batch.argtypes = [vp, vp, vp, i32, i32, vp]
    lib.vhp_sweep_maps_batch_device.argtypes = [vp, vp, vp, i32, i32, vp]
    lib.vhp_planner_solve.argtypes = [vp, i32, i32, i32, i32, f64, u64, vp, vp, vp, vp, C.POINTER(u32)]
    lib.vhp_reconstruct_path.argtypes = [vp, vp, u32, i32, i32, i32, i32, vp, u32, C.POINTER(u32), C.POINTER(f64)]
    lib.vhp_set_option.argtypes = [vp, C.c_char_p, C.c_longlong]
    lib.vhp_planner_solve_speculative.argtypes = [vp, i32, i32, i32, i32, f64, u64, i32, i32, vp, vp, vp, vp, C.POINTER(u32), vp]
    lib.vhp_planner_solve_device.argtypes = [vp, i32, i32, i32, i32, f64, u64, C.POINTER(u32)]
    lib.vhp_planner_results_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.vhp_planner_solve_batch.argtypes = [vp, vp, vp, i32, u64, vp, vp]
    lib.vhp_planner_batch_results_device.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.vhp_planner_batch_results.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.vhp_planner_batch_group.argtypes = [vp]
    lib.vhp_planner_solve_maps_batch.argtypes = [vp, vp, vp, vp, i32, u64, vp, vp]
    lib.vhp_planner_maps_batch_results_device.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.vhp_planner_maps_batch_results.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.vhp_planner_maps_batch_group.argtypes = [vp]
    for name in ("vhp_planner_batch_paths", "vhp_planner_maps_batch_paths", "vhp_planner_path"):
        getattr(lib, name).argtypes = [vp, vp, u32, vp, vp, vp]
        getattr(lib, name + "_device").argtypes = [vp, vp, u32, vp, vp, vp]
    for name in ("vhp_planner_length_fields", "vhp_planner_length_fields_device"):
        getattr(lib, name).argtypes = [vp, i32, i32, i32, vp, vp]
    for name in ("vhp_planner_goal_paths", "vhp_planner_goal_paths_device"):
        getattr(lib, name).argtypes = [vp, i32, vp, i32, vp, u32, vp, vp, vp]
    lib.vhp_sweep_batch_variant.argtypes = [vp, vp, i32, f64, f64, vp]
    lib.vhp_planner_solve_variant.argtypes = [vp, i32, i32, i32, i32, f64, f64, u64, vp, vp, vp, vp, C.POINTER(u32)]
    lib.vhp_sweep_batch_offset.argtypes = [vp, vp, i32, f64, vp]
    lib.vhp_raycast_all.argtypes = [vp, i32, i32, vp]
    lib.vhp_raycast_batch.argtypes = [vp, vp, i32, i32, vp]
    lib.vhp_raycast_batch_device.argtypes = [vp, vp, i32, i32, vp]
    lib.vhp_raycast_maps_batch.argtypes = [vp, vp, vp, i32, i32, vp]
    lib.vhp_raycast_maps_batch_device.argtypes = [vp, vp, vp, i32, i32, vp]
    lib.vhp_line_of_sight.argtypes = [vp, vp, i32, vp]
    lib.vhp_line_of_sight_device.argtypes = [vp, vp, i32, vp]
    lib.vhp_timing.argtypes = [vp, i32]
    lib.vhp_timing_collect.argtypes = [vp, vp, i32, C.POINTER(i32)]
    lib.vhp_last_elapsed_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.vhp_version.restype = C.c_char_p
    lib.vhp_last_sweep_kernel.argtypes = [vp]
    lib.vhp_probe_stores.argtypes = [vp, vp, C.c_ulonglong, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.vhp_alloc_output.argtypes = [vp, C.c_ulonglong, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]
    lib.vhp_free_output.argtypes = [vp, vp]
    lib.vhp_alloc_output_cost.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)]
    lib.vhp_multi_create.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]
    lib.vhp_multi_destroy.argtypes = [vp]
    lib.vhp_multi_last_error.argtypes = [vp]
    lib.vhp_multi_last_error.restype = C.c_char_p
    lib.vhp_multi_devices.argtypes = [vp]
    lib.vhp_multi_context.argtypes = [vp, i32]
    lib.vhp_multi_context.restype = vp
    lib.vhp_multi_shard_bounds.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.vhp_multi_shard_bounds.restype = None
    lib.vhp_multi_set_map.argtypes = [vp, vp, i32, i32]
    lib.vhp_multi_sweep_batch.argtypes = [vp, vp, i32, i32, i32, C.POINTER(vp)]
    lib.vhp_multi_allgather_fields.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(vp)]
    lib.vhp_multi_allgather_plan.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32]
    lib.vhp_multi_use_rccl.argtypes = [vp, i32]
    lib.vhp_union_fields_device.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    lib.vhp_union_partials_device.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    lib.vhp_multi_union_fields.argtypes = [vp, i32, i32, vp, vp, vp]
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One GPU, one occupancy map.  Mirrors the lifetime of vbs::visibilityBasedSolver."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.vhp_create(int(device), C.byref(h))
        if rc != VHP_OK:
            raise VhpError(rc, "vhp_create failed (no usable HIP device %d?)" % device)
        self.h = h
        self.nx = self.ny = 0
        self.stream = 0           # the stream handle last given to set_stream (0: the default stream)
        self.field_stride = 0     # the "field_stride" option as last set (vhp_set_map resets it to 0)
        self.n_maps = self.maps_nx = self.maps_ny = 0  # the stack of maps of set_maps
        # (queries, largest n_pivots + 2) of the last batch / maps batch, and the latter of the last plain solve: the path calls' defaults
        self._batch_q = self._maps_batch_q = (1, 2)
        self._path_cap = 2

    def close(self):
        if getattr(self, "h", None):
            self.lib.vhp_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc, ok=(VHP_OK,)):
        if rc not in ok:
            raise VhpError(rc, (self.lib.vhp_last_error(self.h) or b"").decode())
        return rc

    def set_stream(self, stream_handle):
        self._check(self.lib.vhp_set_stream(self.h, C.c_void_p(stream_handle or 0)))
        self.stream = stream_handle or 0

    def set_map(self, occ):
        occ = np.ascontiguousarray(occ, np.uint8)
        self.ny, self.nx = occ.shape
        self._check(self.lib.vhp_set_map(self.h, _ptr(occ), self.nx, self.ny))
        self.field_stride = 0

    def set_map_device(self, dptr, nx, ny):
        self.nx, self.ny = nx, ny
        self._check(self.lib.vhp_set_map_device(self.h, C.c_void_p(dptr), nx, ny))
        self.field_stride = 0

    def sweep_batch(self, sources, variant=SWEEP_FULL, dtype=F64):
        """Host-buffer form.  sources int32 [n, 2] (x, y) -> fields [n, ny, nx]."""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
        out = np.empty((len(src), self.ny, self.nx), np.float64 if dtype == F64 else np.float32)
        self._check(self.lib.vhp_sweep_batch(self.h, _ptr(src), len(src), variant, dtype, _ptr(out)))
        return out

    def sweep_batch_device(self, d_src, n_src, d_out, variant=SWEEP_FULL, dtype=F64):
        """Device-resident, asynchronous on the context stream.  d_src / d_out are raw device pointers."""
        self._check(self.lib.vhp_sweep_batch_device(self.h, C.c_void_p(d_src), n_src, variant, dtype, C.c_void_p(d_out)))

    def set_maps(self, occ):
        """A stack of maps of one size, uint8 [M, ny, nx] (1 = free): state of its own, beside the map of set_map."""
        occ = np.ascontiguousarray(occ, np.uint8)
        if occ.ndim != 3:
            raise ValueError("set_maps: occ must be [n_maps, ny, nx], got shape %r" % (occ.shape,))
        m, ny, nx = occ.shape
        self.n_maps = self.maps_nx = self.maps_ny = 0
        self._check(self.lib.vhp_set_maps(self.h, _ptr(occ), m, nx, ny))
        self.n_maps, self.maps_nx, self.maps_ny = m, nx, ny

    def set_maps_device(self, dptr, n_maps, nx, ny):
        """Same, the maps already in device memory (raw pointer)."""
        self.n_maps = self.maps_nx = self.maps_ny = 0
        self._check(self.lib.vhp_set_maps_device(self.h, C.c_void_p(dptr), n_maps, nx, ny))
        self.n_maps, self.maps_nx, self.maps_ny = n_maps, nx, ny

    def set_maps_windows(self, origins, w, h):
        """vhp_set_maps_windows: the stack of maps as windows of the map of set_map, cut on the device.  origins int32 [n, 2] (x, y):
        window k is the w x h cells from origins[k] on, blocked where they lie outside the grid (any int32 origin is valid).
        Replaces the stack of set_maps; everything that runs on a stack then runs on the windows, in window coordinates (adding
        the origin back to sources, queries, paths and hit cells is the caller's job)."""
        org = np.ascontiguousarray(origins, np.int32).reshape(-1, 2)
        self.n_maps = self.maps_nx = self.maps_ny = 0
        self._check(self.lib.vhp_set_maps_windows(self.h, _ptr(org), len(org), int(w), int(h)))
        self.n_maps, self.maps_nx, self.maps_ny = len(org), int(w), int(h)

    def set_maps_windows_device(self, d_origins, n, w, h):
        """Same, the origins (int32 [n, 2]) already in device memory (raw pointer)."""
        self.n_maps = self.maps_nx = self.maps_ny = 0
        self._check(self.lib.vhp_set_maps_windows_device(self.h, C.c_void_p(d_origins), int(n), int(w), int(h)))
        self.n_maps, self.maps_nx, self.maps_ny = int(n), int(w), int(h)

    def maps_occupancy(self, first=0, n=None):
        """vhp_maps_occupancy: maps first .. first + n - 1 of the stack (default: all from `first`) as uint8 [n, maps_ny, maps_nx],
        1 = free -- what set_maps would take."""
        n = self.n_maps - int(first) if n is None else int(n)
        out = np.empty((max(n, 0), self.maps_ny, self.maps_nx), np.uint8)
        self._check(self.lib.vhp_maps_occupancy(self.h, int(first), n, _ptr(out)))
        return out

    def maps_occupancy_device(self, d_out, first=0, n=None):
        """Device-resident, asynchronous on the context stream.  d_out is a raw device pointer to n * maps_ny * maps_nx bytes."""
        n = self.n_maps - int(first) if n is None else int(n)
        self._check(self.lib.vhp_maps_occupancy_device(self.h, int(first), n, C.c_void_p(d_out)))

    def inflate_map(self, radius=None, shape="disc", p=None, border=False):
        """vhp_inflate_map: the map of set_map replaced by its inflation by a robot's footprint, on the device -- a cell is blocked
        afterwards exactly when the footprint around it touches a blocked cell.  The footprint as in `footprint` (one of radius and
        p; a reach of at most MAX_INFLATE cells); cells outside the grid are free, or blocked with border=True.  The context is then
        as after set_map_device of the inflated map (field_stride 0, the solves on the single map dropped, the stack untouched).
        Inflate BEFORE cutting windows (set_maps_windows): a window of the inflated map knows the obstacles just outside it, an
        inflated window does not."""
        s, p = footprint(radius, shape, p)
        self._check(self.lib.vhp_inflate_map(self.h, s, p, INFLATE_BORDER if border else 0))
        self.field_stride = 0

    def inflate_maps(self, first=0, n=None, radius=None, shape="disc", p=None, border=False):
        """vhp_inflate_maps: the same for maps first .. first + n - 1 of the stack (default: all from `first`), the others left as
        they are; the results of a maps batch are dropped.  K robot sizes on one map: set_maps_windows([(0, 0)] * K, nx, ny),
        inflate_maps(k, 1, ...) per size, planner_solve_maps_batch with map_index[q] the class of query q's robot."""
        s, p = footprint(radius, shape, p)
        n = self.n_maps - int(first) if n is None else int(n)
        try:
            self._check(self.lib.vhp_inflate_maps(self.h, int(first), n, s, p, INFLATE_BORDER if border else 0))
        except VhpError as e:
            if e.code == VHP_ERR_HIP:   # (the library leaves no stack behind a failed HIP call)
                self.n_maps = self.maps_nx = self.maps_ny = 0
            raise

    def map_occupancy(self):
        """vhp_map_occupancy: the map of set_map as uint8 [ny, nx], normalised to 1 = free, 0 = blocked -- what shows an inflated map."""
        out = np.empty((self.ny, self.nx), np.uint8)
        self._check(self.lib.vhp_map_occupancy(self.h, _ptr(out)))
        return out

    def map_occupancy_device(self, d_out):
        """Device-resident, asynchronous on the context stream.  d_out is a raw device pointer to ny * nx bytes."""
        self._check(self.lib.vhp_map_occupancy_device(self.h, C.c_void_p(d_out)))

    def map_clearance(self, radius=None, shape="disc", p=None, border=False):
        """vhp_map_clearance: the clearance field of the map of set_map as uint16 [ny, nx] -- per cell the smallest footprint
        parameter at which inflate_map would block it (a disc: the squared distance to the nearest blocked cell; a square or a
        diamond: that distance in their metric), 0 on a blocked cell, CLEARANCE_FAR where it is above p_max.  The footprint as in
        `footprint` names p_max (one of radius and p; a reach of at most MAX_INFLATE cells); cells outside the grid are free, or
        blocked with border=True.  (field > p) is map_occupancy() after inflate_map(p=p) for every p <= p_max: a robot of squared
        radius p fits at a cell exactly when field > p there.  Changes no state."""
        s, p = footprint(radius, shape, p)
        out = np.empty((self.ny, self.nx), np.uint16)
        self._check(self.lib.vhp_map_clearance(self.h, s, p, INFLATE_BORDER if border else 0, _ptr(out)))
        return out

    def map_clearance_device(self, d_out, radius=None, shape="disc", p=None, border=False):
        """Device-resident, asynchronous on the context stream.  d_out is a raw device pointer to ny * nx uint16."""
        s, p = footprint(radius, shape, p)
        self._check(self.lib.vhp_map_clearance_device(self.h, s, p, INFLATE_BORDER if border else 0, C.c_void_p(d_out)))

    def maps_clearance(self, first=0, n=None, radius=None, shape="disc", p=None, border=False):
        """vhp_maps_clearance: the same for maps first .. first + n - 1 of the stack (default: all from `first`), every map by
        itself, as uint16 [n, maps_ny, maps_nx]."""
        s, p = footprint(radius, shape, p)
        n = self.n_maps - int(first) if n is None else int(n)
        out = np.empty((max(n, 0), self.maps_ny, self.maps_nx), np.uint16)
        self._check(self.lib.vhp_maps_clearance(self.h, int(first), n, s, p, INFLATE_BORDER if border else 0, _ptr(out)))
        return out

    def maps_clearance_device(self, d_out, first=0, n=None, radius=None, shape="disc", p=None, border=False):
        """Device-resident, asynchronous on the context stream, one launch whatever n.  d_out is a raw device pointer to
        n * maps_ny * maps_nx uint16; map first + k goes to element k * maps_ny * maps_nx."""
        s, p = footprint(radius, shape, p)
        n = self.n_maps - int(first) if n is None else int(n)
        self._check(self.lib.vhp_maps_clearance_device(self.h, int(first), n, s, p, INFLATE_BORDER if border else 0, C.c_void_p(d_out)))

    def sweep_windows(self, sources, radius, dtype=F64):
        """Range-limited sweeps around many sources of the map of set_map: sets windows of side 2 * radius + 1 with origin
        source - radius (set_maps_windows: this REPLACES the stack of maps) and returns sweep_maps_batch of the local source
        (radius, radius) on window i -- fields [n, 2 * radius + 1, 2 * radius + 1] in window coordinates, field i's cell (a, b) being
        the map's cell sources[i] - radius + (a, b).  Away from its first row and column -- the reference's zeros on whatever grid
        it sweeps (unless the source lies on them), so ask for radius + 1 -- and from the grid's first row and column, every cell
        inside the grid holds, bit for bit, what sweep_batch on the whole map holds there; cells outside the grid are blocked."""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
        r = int(radius)
        if r < 0:
            raise ValueError("sweep_windows: radius must be >= 0, got %d" % r)
        side = 2 * r + 1
        self.set_maps_windows((src.astype(np.int64) - r).astype(np.int32), side, side)
        return self.sweep_maps_batch(np.full((len(src), 2), r, np.int32), np.arange(len(src), dtype=np.int32), dtype)

    def sweep_maps_batch(self, sources, map_index, dtype=F64):
        """Host-buffer form.  sources int32 [n, 2] (x, y), map_index int32 [n] (the map of each source) -> fields [n, ny, nx]."""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
        idx = np.ascontiguousarray(map_index, np.int32).reshape(-1)
        if len(idx) != len(src):
            raise ValueError("sweep_maps_batch: %d sources but %d map indices" % (len(src), len(idx)))
        out = np.empty((len(src), self.maps_ny, self.maps_nx), np.float64 if dtype == F64 else np.float32)
        self._check(self.lib.vhp_sweep_maps_batch(self.h, _ptr(src), _ptr(idx), len(src), dtype, _ptr(out)))
        return out

    def sweep_maps_batch_device(self, d_src, d_map, n_src, d_out, dtype=F64):
        """Device-resident, asynchronous on the context stream.  d_src / d_map / d_out are raw device pointers."""
        self._check(self.lib.vhp_sweep_maps_batch_device(self.h, C.c_void_p(d_src), C.c_void_p(d_map), n_src, dtype, C.c_void_p(d_out)))

    def union_fields_device(self, d_fields, n_fields, d_best, d_arg, first_index=0, dtype=F64):
        """Max-union of n_fields device-resident fields and the (lowest) source index that attains it, into d_best / d_arg (int32);
        raw device pointers, asynchronous on the context stream (include/vhp.h vhp_union_fields_device)."""
        self._check(self.lib.vhp_union_fields_device(self.h, C.c_void_p(d_fields), n_fields, dtype, first_index, C.c_void_p(d_best), C.c_void_p(d_arg)))

    def union_partials_device(self, d_bests, d_args, n_parts, d_best, d_arg, dtype=F64):
        """The same reduction over partial unions with their label fields (vhp_union_partials_device)."""
        self._check(self.lib.vhp_union_partials_device(self.h, C.c_void_p(d_bests), C.c_void_p(d_args), n_parts, dtype, C.c_void_p(d_best), C.c_void_p(d_arg)))

    def sync(self):
        self._check(self.lib.vhp_sync(self.h))

    def set_option(self, key, value):
        """Launch-shape override (include/vhp.h vhp_set_option); 0 / -1 = automatic."""
        self._check(self.lib.vhp_set_option(self.h, key.encode(), int(value)))
        if key == "field_stride":
            self.field_stride = int(value)

    def last_sweep_kernel(self):
        """1 = front sweep, 3 = pool sweep, 4 = latency sweep: what the last batch sweep (or planner solve) launched."""
        return int(self.lib.vhp_last_sweep_kernel(self.h))

    def timing(self, enable=True, prealloc=0):
        """prealloc > 1: room for that many timed launches made now (slots for the timestamps the pool and latency sweeps write, event
        pairs for the other kernels), so that launches inside a timed loop allocate and create nothing."""
        self._check(self.lib.vhp_timing(self.h, max(int(prealloc), 1) if enable else 0))

    def timing_collect(self, cap=4096):
        """Durations (ms) of the sweep kernels launched since timing(True), oldest first."""
        buf = np.zeros(cap, np.float32)
        n = C.c_int(0)
        self._check(self.lib.vhp_timing_collect(self.h, _ptr(buf), cap, C.byref(n)))
        return buf[: n.value].copy()

    def probe_stores(self, d_ptr, n_bytes):
        """(whole-line TB/s, split-line TB/s) of the memory behind a device buffer (vhp_probe_stores; overwrites it)."""
        a, b = C.c_float(0), C.c_float(0)
        self._check(self.lib.vhp_probe_stores(self.h, C.c_void_p(d_ptr), int(n_bytes), C.byref(a), C.byref(b)))
        return a.value, b.value

    def alloc_output(self, n_bytes, max_candidates=24):
        """(device pointer, whole-line TB/s, split-line TB/s, allocations tried): a result buffer placed by the library (vhp_alloc_output)."""
        p, a, b, n = C.c_void_p(), C.c_float(0), C.c_float(0), C.c_int(0)
        self._check(self.lib.vhp_alloc_output(self.h, int(n_bytes), int(max_candidates), C.byref(p), C.byref(a), C.byref(b), C.byref(n)))
        return p.value, a.value, b.value, n.value

    def alloc_output_cost(self):
        """(wall-clock ms, peak bytes held) of the last alloc_output of this context (vhp_alloc_output_cost)."""
        ms, peak = C.c_double(0), C.c_ulonglong(0)
        self._check(self.lib.vhp_alloc_output_cost(self.h, C.byref(ms), C.byref(peak)))
        return ms.value, peak.value

    def free_output(self, d_ptr):
        self._check(self.lib.vhp_free_output(self.h, C.c_void_p(d_ptr)))

    def last_elapsed_ms(self):
        ms = C.c_float(0)
        self._check(self.lib.vhp_last_elapsed_ms(self.h, C.byref(ms)))
        return ms.value

    def planner_solve(self, start, end, threshold, max_iter):
        n = self.nx * self.ny
        came = np.empty((self.ny, self.nx), np.uint64)
        vg = np.empty((self.ny, self.nx), np.float64)
        vl = np.empty((self.ny, self.nx), np.float64)
        piv = np.zeros((int(max_iter) + 2, 2), np.int32)
        npiv = C.c_uint32(0)
        rc = self.lib.vhp_planner_solve(self.h, start[0], start[1], end[0], end[1], float(threshold), int(max_iter),
                                        _ptr(came), _ptr(vg), _ptr(vl), _ptr(piv), C.byref(npiv))
        self._path_cap = npiv.value + 2
        if rc in (VHP_ERR_HIP, VHP_ERR_NO_MAP, VHP_ERR_ARG, VHP_ERR_TOO_LARGE):
            self._check(rc)
        return dict(status=rc, came_from=came, vis_global=vg, vis_local=vl, pivots=piv[: npiv.value + 1].copy(),
                    n_pivots=npiv.value)

    def planner_solve_speculative(self, start, end, threshold, max_iter, k=4, mode=0, outputs=True):
        """vhp_planner_solve_speculative: mode 0 = exact (same outputs as planner_solve), mode 1 = fast (commits all k).
        Adds stats: cache hits, sweeping iterations, fields swept."""
        came = np.empty((self.ny, self.nx), np.uint64) if outputs else None
        vg = np.empty((self.ny, self.nx), np.float64) if outputs else None
        vl = np.empty((self.ny, self.nx), np.float64) if outputs else None
        piv = np.zeros((int(max_iter) + 2 + 8, 2), np.int32)
        npiv = C.c_uint32(0)
        st = np.zeros(3, np.int32)
        rc = self.lib.vhp_planner_solve_speculative(self.h, start[0], start[1], end[0], end[1], float(threshold), int(max_iter), int(k), int(mode),
                                                    _ptr(came) if outputs else None, _ptr(vg) if outputs else None, _ptr(vl) if outputs else None,
                                                    _ptr(piv), C.byref(npiv), _ptr(st))
        self._path_cap = npiv.value + 2
        if rc in (VHP_ERR_HIP, VHP_ERR_NO_MAP, VHP_ERR_ARG, VHP_ERR_TOO_LARGE):
            self._check(rc)
        return dict(status=rc, came_from=came, vis_global=vg, vis_local=vl, pivots=piv[: npiv.value + 1].copy(), n_pivots=npiv.value,
                    hits=int(st[0]), sweeps=int(st[1]), fields_swept=int(st[2]))

    def planner_solve_device(self, start, end, threshold, max_iter):
        """Planner solve with the results left on the device.  Returns (status, n_pivots, dict of raw device pointers:
        labels uint32 [ny, nx] (0xFFFFFFFF = unlabelled), vis_global / vis_local float64 [ny, nx], pivots int32 [n_pivots+1, 2])."""
        npiv = C.c_uint32(0)
        rc = self.lib.vhp_planner_solve_device(self.h, start[0], start[1], end[0], end[1], float(threshold), int(max_iter), C.byref(npiv))
        self._path_cap = npiv.value + 2
        if rc in (VHP_ERR_HIP, VHP_ERR_NO_MAP, VHP_ERR_ARG, VHP_ERR_TOO_LARGE):
            self._check(rc)
        ptrs = {}
        if rc in (VHP_OK, VHP_ERR_MAX_ITER):
            p = [C.c_void_p() for _ in range(4)]
            self._check(self.lib.vhp_planner_results_device(self.h, *[C.byref(q) for q in p]))
            ptrs = dict(labels=p[0].value, vis_global=p[1].value, vis_local=p[2].value, pivots=p[3].value)
        return rc, npiv.value, ptrs

    def planner_solve_batch(self, queries, thresholds, max_iter, outputs=True):
        """vhp_planner_solve_batch: Q independent planner_solve calls on this map in one call.  queries: [Q, 4] (start_x, start_y,
        end_x, end_y), field coordinates; thresholds: Q values or one for all.  Returns one dict per query with planner_solve's keys
        and dtypes (outputs=False: status and n_pivots only; outputs="paths": status, n_pivots, path_status, length and path -- the path
        reconstructed on the device, no field copied: vhp_planner_batch_paths).  A query that failed validation has pivots [[0, 0]] and None for
        came_from, vis_global and vis_local, as it has no results."""
        q = np.ascontiguousarray(queries, np.int32).reshape(-1, 4)
        n = len(q)
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, np.float64), (n,)))
        st = np.zeros(n, np.int32)
        npiv = np.zeros(n, np.uint32)
        self._check(self.lib.vhp_planner_solve_batch(self.h, _ptr(q), _ptr(thr), n, int(max_iter), _ptr(st), _ptr(npiv)))
        self._batch_q = (n, int(npiv.max()) + 2)
        if outputs == "paths":
            return self._batch_with_paths(st, npiv, self.lib.vhp_planner_batch_paths)
        return self._batch_outputs(st, npiv, outputs, self.nx, self.ny, self.lib.vhp_planner_batch_results)

    def _paths(self, call, n, cap):
        """One host-form path call (include/vhp.h vhp_planner_batch_paths) for n queries: a list of dict(status, length, n_path, path)
        (n_path: the point count, also where cap was too small for it)."""
        cap = int(cap)
        xy = np.zeros((n, max(cap, 1), 2), np.int32)
        cnt = np.zeros(n, np.uint32)
        length = np.zeros(n, np.float64)
        st = np.zeros(n, np.int32)
        self._check(call(self.h, _ptr(xy), cap, _ptr(cnt), _ptr(length), _ptr(st)))
        return [dict(status=int(st[q]), length=float(length[q]), n_path=int(cnt[q]),
                     path=xy[q, : int(cnt[q])].copy() if st[q] == VHP_OK else np.zeros((0, 2), np.int32)) for q in range(n)]

    def _batch_with_paths(self, st, npiv, call):
        paths = self._paths(call, len(st), int(npiv.max()) + 2)
        return [dict(status=int(st[q]), n_pivots=int(npiv[q]), path_status=p["status"], length=p["length"], path=p["path"])
                for q, p in enumerate(paths)]

    def planner_batch_paths(self, cap=None):
        """vhp_planner_batch_paths: the paths of the queries of the last planner_solve_batch, reconstructed on the device.  A list of
        dict(status, length, path) -- path int32 [n_path, 2], start first, empty where status is not VHP_OK.  cap: points of room per
        query (default: the largest n_pivots + 2 of the solve)."""
        n, dflt = self._batch_q
        return self._paths(self.lib.vhp_planner_batch_paths, n, dflt if cap is None else cap)

    def planner_batch_paths_device(self, d_path_xy, cap, d_n_path=0, d_length=0, d_status=0):
        """vhp_planner_batch_paths_device: raw device pointers (0: not wanted), asynchronous on the context stream."""
        self._check(self.lib.vhp_planner_batch_paths_device(self.h, C.c_void_p(d_path_xy or None), int(cap), C.c_void_p(d_n_path or None),
                                                            C.c_void_p(d_length or None), C.c_void_p(d_status or None)))

    def planner_maps_batch_paths(self, cap=None):
        """vhp_planner_maps_batch_paths: planner_batch_paths for the last planner_solve_maps_batch."""
        n, dflt = self._maps_batch_q
        return self._paths(self.lib.vhp_planner_maps_batch_paths, n, dflt if cap is None else cap)

    def planner_maps_batch_paths_device(self, d_path_xy, cap, d_n_path=0, d_length=0, d_status=0):
        """vhp_planner_maps_batch_paths_device (see planner_batch_paths_device)."""
        self._check(self.lib.vhp_planner_maps_batch_paths_device(self.h, C.c_void_p(d_path_xy or None), int(cap), C.c_void_p(d_n_path or None),
                                                                 C.c_void_p(d_length or None), C.c_void_p(d_status or None)))

    def planner_path(self, cap=None):
        """vhp_planner_path: the path of the last planner_solve / planner_solve_device / planner_solve_speculative, reconstructed on
        the device: dict(status, length, path)."""
        return self._paths(self.lib.vhp_planner_path, 1, self._path_cap if cap is None else cap)[0]

    def planner_path_device(self, d_path_xy, cap, d_n_path=0, d_length=0, d_status=0):
        """vhp_planner_path_device (see planner_batch_paths_device)."""
        self._check(self.lib.vhp_planner_path_device(self.h, C.c_void_p(d_path_xy or None), int(cap), C.c_void_p(d_n_path or None),
                                                     C.c_void_p(d_length or None), C.c_void_p(d_status or None)))

    def _solve_kind(self, solve):
        """(vhp_solve_kind, queries of that solve, its default path room, nx, ny) for solve = "plain" | "batch" | "maps" (or the constant)"""
        kind = _SOLVE_KINDS[solve] if isinstance(solve, str) else int(solve)
        if kind == SOLVE_PLAIN:
            return kind, 1, self._path_cap, self.nx, self.ny
        if kind == SOLVE_BATCH:
            return (kind,) + tuple(self._batch_q) + (self.nx, self.ny)
        if kind == SOLVE_MAPS_BATCH:
            return (kind,) + tuple(self._maps_batch_q) + (self.maps_nx, self.maps_ny)
        raise ValueError("solve must be 'plain', 'batch' or 'maps', got %r" % (solve,))

    def planner_length_fields(self, solve="plain", q_first=0, n_q=None):
        """vhp_planner_length_fields: for queries q_first .. q_first + n_q - 1 of a solve (default: all from q_first) the path length from
        the query's start to EVERY cell and that path's point count, read off the tree the solve left on the device.  Returns (length
        float64 [n_q, ny, nx], n_path uint32 [n_q, ny, nx]); a cell the solve did not reach has length -1.0 and n_path 0."""
        kind, n, _, nx, ny = self._solve_kind(solve)
        n_q = n - int(q_first) if n_q is None else int(n_q)
        length = np.empty((max(n_q, 0), ny, nx), np.float64)
        cnt = np.empty((max(n_q, 0), ny, nx), np.uint32)
        self._check(self.lib.vhp_planner_length_fields(self.h, kind, int(q_first), n_q, _ptr(length), _ptr(cnt)))
        return length, cnt

    def planner_length_fields_device(self, d_length, d_n_path=0, solve="plain", q_first=0, n_q=None):
        """vhp_planner_length_fields_device: raw device pointers (0: not wanted), asynchronous on the context stream."""
        kind, n, _, _, _ = self._solve_kind(solve)
        n_q = n - int(q_first) if n_q is None else int(n_q)
        self._check(self.lib.vhp_planner_length_fields_device(self.h, kind, int(q_first), n_q, C.c_void_p(d_length or None), C.c_void_p(d_n_path or None)))

    def planner_goal_paths(self, goals, solve="plain", cap=None):
        """vhp_planner_goal_paths: the path from a query's start to each goal -- goals int32 [n, 3] rows (q, x, y) -- reconstructed on the
        device.  A list of dict(status, length, n_path, path) as planner_batch_paths gives per query.  cap: points of room per goal
        (default: the largest n_pivots + 2 of the solve, enough for any cell)."""
        kind, _, dflt, _, _ = self._solve_kind(solve)
        g = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
        call = lambda h, xy, cap, cnt, length, st: self.lib.vhp_planner_goal_paths(h, kind, _ptr(g), len(g), xy, cap, cnt, length, st)
        return self._paths(call, len(g), dflt if cap is None else cap)

    def planner_goal_paths_device(self, d_goals, n_goals, d_path_xy, cap, d_n_path=0, d_length=0, d_status=0, solve="plain"):
        """vhp_planner_goal_paths_device: raw device pointers (0: not wanted), asynchronous on the context stream."""
        kind = self._solve_kind(solve)[0]
        self._check(self.lib.vhp_planner_goal_paths_device(self.h, kind, C.c_void_p(d_goals or None), int(n_goals), C.c_void_p(d_path_xy or None),
                                                           int(cap), C.c_void_p(d_n_path or None), C.c_void_p(d_length or None),
                                                           C.c_void_p(d_status or None)))

    def _batch_outputs(self, st, npiv, outputs, nx, ny, results):
        n = len(st)
        out = []
        for k in range(n):
            r = dict(status=int(st[k]), n_pivots=int(npiv[k]))
            if outputs:
                solved = r["status"] in (VHP_OK, VHP_ERR_MAX_ITER, VHP_ERR_NOTHING_LIT)
                piv = np.zeros((r["n_pivots"] + 1, 2), np.int32)
                came = vg = vl = None
                if solved:
                    came = np.empty((ny, nx), np.uint64)
                    vg = np.empty((ny, nx), np.float64)
                    vl = np.empty((ny, nx), np.float64)
                    self._check(results(self.h, k, _ptr(came), _ptr(vg), _ptr(vl), _ptr(piv)))
                r.update(came_from=came, vis_global=vg, vis_local=vl, pivots=piv)
            out.append(r)
        return out

    def planner_batch_results_device(self, q):
        """Raw device pointers of query q of the last planner_solve_batch: labels uint32 [ny, nx], vis_global / vis_local float64
        [ny, nx], pivots int32 [n_pivots + 1, 2] (vhp_planner_batch_results_device)."""
        p = [C.c_void_p() for _ in range(4)]
        self._check(self.lib.vhp_planner_batch_results_device(self.h, int(q), *[C.byref(v) for v in p]))
        return dict(labels=p[0].value, vis_global=p[1].value, vis_local=p[2].value, pivots=p[3].value)

    def planner_batch_group(self):
        """Queries per group of the last planner_solve_batch (0: none yet)."""
        return int(self.lib.vhp_planner_batch_group(self.h))

    def planner_solve_maps_batch(self, queries, map_index, thresholds, max_iter, outputs=True):
        """vhp_planner_solve_maps_batch: planner_solve_batch across the stack of set_maps -- query q on map map_index[q].  Returns
        planner_solve_batch's list of dicts (fields [maps_ny, maps_nx])."""
        q = np.ascontiguousarray(queries, np.int32).reshape(-1, 4)
        idx = np.ascontiguousarray(map_index, np.int32).reshape(-1)
        if len(idx) != len(q):
            raise ValueError("planner_solve_maps_batch: %d queries but %d map indices" % (len(q), len(idx)))
        n = len(q)
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, np.float64), (n,)))
        st = np.zeros(n, np.int32)
        npiv = np.zeros(n, np.uint32)
        self._check(self.lib.vhp_planner_solve_maps_batch(self.h, _ptr(q), _ptr(idx), _ptr(thr), n, int(max_iter), _ptr(st), _ptr(npiv)))
        self._maps_batch_q = (n, int(npiv.max()) + 2)
        if outputs == "paths":
            return self._batch_with_paths(st, npiv, self.lib.vhp_planner_maps_batch_paths)
        return self._batch_outputs(st, npiv, outputs, self.maps_nx, self.maps_ny, self.lib.vhp_planner_maps_batch_results)

    def planner_maps_batch_results_device(self, q):
        """Raw device pointers of query q of the last planner_solve_maps_batch (the layout of planner_batch_results_device)."""
        p = [C.c_void_p() for _ in range(4)]
        self._check(self.lib.vhp_planner_maps_batch_results_device(self.h, int(q), *[C.byref(v) for v in p]))
        return dict(labels=p[0].value, vis_global=p[1].value, vis_local=p[2].value, pivots=p[3].value)

    def planner_maps_batch_group(self):
        """Queries per group of the last planner_solve_maps_batch (0: none yet)."""
        return int(self.lib.vhp_planner_maps_batch_group(self.h))

    def sweep_batch_variant(self, sources, alpha=1.0, fac=1.0):
        """MATLAB-flavoured sweep (getAccessibilityMap.m): fields [n, ny, nx] float64."""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
        out = np.empty((len(src), self.ny, self.nx), np.float64)
        self._check(self.lib.vhp_sweep_batch_variant(self.h, _ptr(src), len(src), float(alpha), float(fac), _ptr(out)))
        return out

    def sweep_batch_offset(self, sources, offset):
        """computeVisibility() with the reference's `offset` local exposed (include/vhp.h): fields [n, ny, nx] float64."""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
        out = np.empty((len(src), self.ny, self.nx), np.float64)
        self._check(self.lib.vhp_sweep_batch_offset(self.h, _ptr(src), len(src), float(offset), _ptr(out)))
        return out

    def planner_solve_variant(self, start, end, threshold, alpha, max_iter):
        lab = np.empty((self.ny, self.nx), np.uint64)
        uni = np.empty((self.ny, self.nx), np.float64)
        loc = np.empty((self.ny, self.nx), np.float64)
        way = np.zeros((int(max_iter) + 3, 2), np.int32)
        n = C.c_uint32(0)
        rc = self.lib.vhp_planner_solve_variant(self.h, start[0], start[1], end[0], end[1], float(threshold), float(alpha), int(max_iter),
                                                _ptr(lab), _ptr(uni), _ptr(loc), _ptr(way), C.byref(n))
        if rc in (VHP_ERR_HIP, VHP_ERR_NO_MAP, VHP_ERR_ARG, VHP_ERR_TOO_LARGE):
            self._check(rc)
        return dict(status=rc, label=lab, map_builder=uni, local=loc, waypoints=way[: n.value].copy())

    def raycast_all(self, sx, sy):
        out = np.empty((self.ny, self.nx), np.float64)
        self._check(self.lib.vhp_raycast_all(self.h, int(sx), int(sy), _ptr(out)))
        return out

    def raycast_batch(self, sources, dtype=F64):
        """vhp_raycast_batch: the reference's ray-cast field (a Bresenham ray to every cell) for each source in one call.  sources int32
        [n, 2] (x, y) -> fields [n, ny, nx] of float64, float32 or uint8 (dtype F64 / F32 / U8), 1 = visible."""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
        out = np.empty((len(src), self.ny, self.nx), _DTYPES[dtype])
        self._check(self.lib.vhp_raycast_batch(self.h, _ptr(src), len(src), dtype, _ptr(out)))
        return out

    def raycast_batch_device(self, d_src, n_src, d_out, dtype=F64):
        """Device-resident, asynchronous on the context stream.  d_src / d_out are raw device pointers; the fields are packed."""
        self._check(self.lib.vhp_raycast_batch_device(self.h, C.c_void_p(d_src), n_src, dtype, C.c_void_p(d_out)))

    def raycast_maps_batch(self, sources, map_index, dtype=F64):
        """vhp_raycast_maps_batch: raycast_batch across the stack of set_maps -- source i on map map_index[i] -> fields [n, maps_ny, maps_nx]."""
        src = np.ascontiguousarray(sources, np.int32).reshape(-1, 2)
        idx = np.ascontiguousarray(map_index, np.int32).reshape(-1)
        if len(idx) != len(src):
            raise ValueError("raycast_maps_batch: %d sources but %d map indices" % (len(src), len(idx)))
        out = np.empty((len(src), self.maps_ny, self.maps_nx), _DTYPES[dtype])
        self._check(self.lib.vhp_raycast_maps_batch(self.h, _ptr(src), _ptr(idx), len(src), dtype, _ptr(out)))
        return out

    def raycast_maps_batch_device(self, d_src, d_map, n_src, d_out, dtype=F64):
        """Device-resident, asynchronous on the context stream.  d_src / d_map / d_out are raw device pointers."""
        self._check(self.lib.vhp_raycast_maps_batch_device(self.h, C.c_void_p(d_src), C.c_void_p(d_map), n_src, dtype, C.c_void_p(d_out)))

    def line_of_sight(self, pairs):
        """vhp_line_of_sight: pairs int32 [n, 4] rows (x0, y0, x1, y1) -> int32 [n, 2]: the first blocked cell on the reference's ray from
        (x0, y0) to (x1, y1) (the start is tested, the target is not), or (-1, -1) where the segment is clear.  A pair with an end outside
        the grid raises VhpError (VHP_ERR_SOURCE_OOB); the C call marks such rows (-2, -2) and answers the others."""
        p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 4)
        hit = np.empty((len(p), 2), np.int32)
        self._check(self.lib.vhp_line_of_sight(self.h, _ptr(p), len(p), _ptr(hit)))
        return hit

    def line_of_sight_device(self, d_pairs, n_pairs, d_hit):
        """Device-resident, asynchronous on the context stream.  d_pairs (int32 [n, 4]) / d_hit (int32 [n, 2]) are raw device pointers."""
        self._check(self.lib.vhp_line_of_sight_device(self.h, C.c_void_p(d_pairs), n_pairs, C.c_void_p(d_hit)))

    def reconstruct_path(self, came_from, pivots, end):
        return reconstruct_path(came_from, pivots, end)


def reconstruct_path(came_from, pivots, end):
    """vhp_reconstruct_path (host-only: needs no context and no GPU).

    pivots: [n_pivots + 1, 2] as planner_solve returns them (the last entry is `end`).  Returns (length, path)."""
    lib = load_library()
    ny, nx = came_from.shape
    piv = np.ascontiguousarray(pivots, np.int32).reshape(-1, 2)
    n_pivots = len(piv) - 1
    cap = n_pivots + 3
    path = np.zeros((cap, 2), np.int32)
    n = C.c_uint32(0)
    d = C.c_double(0)
    came = np.ascontiguousarray(came_from, np.uint64)
    rc = lib.vhp_reconstruct_path(_ptr(came), _ptr(piv), n_pivots, nx, ny, end[0], end[1], _ptr(path), cap,
                                  C.byref(n), C.byref(d))
    if rc != VHP_OK:
        raise VhpError(rc, "vhp_reconstruct_path: inconsistent came_from / pivots (or a path longer than %d points)" % cap)
    return d.value, path[: n.value].copy()


def version():
    return load_library().vhp_version().decode()
