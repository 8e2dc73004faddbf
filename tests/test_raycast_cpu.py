"""Ray casting for batches of sources, without a GPU: the shared ray walk of csrc/vhp_raycast.hpp -- what the field kernel and the
line-of-sight kernel call -- run by tests/raycast_driver.cpp over maps it packs on the host in the layout of vhp_pack_rows_stack /
vhp_pack_cols_stack, and held byte for byte to oracle.raycast_all; the launch plan's coverage; the step count of a ray against the reference's own loop; the
new symbols in the header and the binding.  The driver is built plain and under the address and undefined-behaviour sanitizers, and
every check runs through both."""
import os
import re
import subprocess

import numpy as np
import pytest

import cpu_driver
import raycast_cases as cases

NEW_SYMBOLS = ["vhp_raycast_batch", "vhp_raycast_batch_device", "vhp_raycast_maps_batch", "vhp_raycast_maps_batch_device",
               "vhp_line_of_sight", "vhp_line_of_sight_device"]


@pytest.fixture(scope="module", params=["plain", "san"])
def driver(request, tmp_path_factory):
    san = request.param == "san"
    return cpu_driver.build(os.path.join(cpu_driver.HERE, "raycast_driver.cpp"), str(tmp_path_factory.mktemp("raycast")),
                            "raycast_driver_" + request.param, flags=() if san else ("-O2",), sanitized=san)


def _fields(exe, occ, sources, tmp_path):
    ny, nx = occ.shape
    path = os.path.join(str(tmp_path), "map_%dx%d.bin" % (nx, ny))
    np.ascontiguousarray(occ, np.uint8).tofile(path)
    p = subprocess.run([exe, "fields", path, str(nx), str(ny)], input="".join("%d %d\n" % s for s in sources).encode(), capture_output=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return np.frombuffer(p.stdout, np.uint8).reshape(len(sources), ny, nx)


@pytest.mark.parametrize("nx,ny,seed", cases.GRIDS)
def test_walk_equals_oracle(driver, oracle, tmp_path, nx, ny, seed):
    occ = cases.grid_map(nx, ny, seed)
    sources = cases.sources_for(occ)
    got = _fields(driver, occ, sources, tmp_path)
    seen = set()
    for k, (sx, sy) in enumerate(sources):
        want = oracle.raycast_all(occ, sx, sy)
        seen |= set(np.unique(want).tolist())
        if seed is not None and occ[sy, sx]:
            assert {0.0, 1.0} <= set(np.unique(want).tolist()), "the case would pass on all-ones: source %r" % ((sx, sy),)
        assert got[k].tobytes() == want.astype(np.uint8).tobytes(), "source %r on %d x %d: %d cells differ" % (
            (sx, sy), nx, ny, int((got[k] != want).sum()))
    assert seen <= {0.0, 1.0}


def test_walk_on_a_map_whose_free_cells_are_255(driver, oracle, tmp_path):
    nx, ny, seed = cases.RECT[3]
    occ = cases.rect_map(nx, ny, seed) * np.uint8(255)
    sources = cases.sources_for(occ)[:6]
    got = _fields(driver, occ, sources, tmp_path)
    for k, (sx, sy) in enumerate(sources):
        want = oracle.raycast_all(occ, sx, sy)
        assert 0.0 in want and 1.0 in want
        assert got[k].tobytes() == want.astype(np.uint8).tobytes(), (sx, sy)


def test_contract_oddities(driver, oracle, tmp_path):
    """A blocked cell in plain sight with nothing behind it stays 1; a blocked source zeroes every cell; 1 x 1 stays 1."""
    occ = np.ones((5, 5), np.uint8)
    occ[4, 4] = occ[0, 2] = 0          # a corner and a border cell
    (got,) = _fields(driver, occ, [(0, 2)], tmp_path)
    want = oracle.raycast_all(occ, 0, 2)
    assert want[4, 4] == 1.0 and want[0, 2] == 1.0 and got.tobytes() == want.astype(np.uint8).tobytes()
    (got,) = _fields(driver, occ, [(4, 4)], tmp_path)
    assert not got.any() and not oracle.raycast_all(occ, 4, 4).any()
    (got,) = _fields(driver, np.ones((1, 1), np.uint8), [(0, 0)], tmp_path)
    assert got.tolist() == [[1]]
    (got,) = _fields(driver, np.zeros((1, 1), np.uint8), [(0, 0)], tmp_path)
    assert got.tolist() == [[1]] and oracle.raycast_all(np.zeros((1, 1), np.uint8), 0, 0).tolist() == [[1.0]]


@pytest.mark.parametrize("n_src", [0, 1, 65535, 65536, 70000])
@pytest.mark.parametrize("cells", [9, 1000])
def test_launch_plan_takes_every_pair_once(driver, cells, n_src):
    p = subprocess.run([driver, "plan", str(cells), str(n_src)], capture_output=True, text=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-2000:])
    tiles, grid_y = (int(v) for v in p.stdout.split())
    assert tiles == (cells + 255) // 256 and grid_y == min(n_src, 65535)


def test_a_ray_takes_max_dx_dy_steps(driver):
    """What lets the walk be a counted loop: exhaustively up to 512, and every dy of the two longest rays a grid allows."""
    p = subprocess.run([driver, "steps", "512"], capture_output=True, text=True, check=False)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
    assert int(p.stdout) == 8 * (513 * 514 // 2)
    for dx in (4095, 8191):
        p = subprocess.run([driver, "steps-of", str(dx)], capture_output=True, text=True, check=False)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
        assert int(p.stdout) == 8 * (dx + 1)


def test_python_ray_equals_oracle(oracle):
    """The restatement the line-of-sight expectations come from: over all targets of a source its zero set is the oracle's field."""
    nx, ny, seed = cases.RECT[0]
    occ = cases.rect_map(nx, ny, seed)
    for sx, sy in cases.sources_for(occ)[:4] + cases.sources_for(occ)[-2:]:
        assert cases.field_from_hits(cases.hits_from(occ, sx, sy)).tobytes() == oracle.raycast_all(occ, sx, sy).tobytes(), (sx, sy)
    assert cases.ray(occ, 5, 5, 5, 5) is None


def test_header_and_binding_name_the_new_entry_points():
    import vhp_amd
    header = open(os.path.join(cpu_driver.INCLUDE, "vhp.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(vhp_ctx\*" % name, header), name
        assert name in vhp_amd.ABI_SYMBOLS, name
    assert re.search(r"VHP_U8\s*=\s*2\b", header) and vhp_amd.U8 == 2
    for method in ("raycast_batch", "raycast_batch_device", "raycast_maps_batch", "raycast_maps_batch_device", "line_of_sight", "line_of_sight_device"):
        assert callable(getattr(vhp_amd.Context, method)), method
