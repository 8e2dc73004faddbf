"""Builds and runs tests/pool_scratch_driver.cpp: the pool sweep's scratch sizes (csrc/vhp_pool_scratch.hpp) against UnitGeo, on the CPU."""
import atexit
import os
import shutil
import subprocess
import tempfile

import cpu_driver

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "visibility-heuristic-path-planner_amd", "csrc")
DRIVER = os.path.join(HERE, "pool_scratch_driver.cpp")

_exes = {}
_dir = None


def driver(sanitized=False):
    """The driver's executable, plain or under the address and undefined-behaviour sanitizers; built once per process."""
    global _dir
    if sanitized not in _exes:
        if _dir is None:
            _dir = tempfile.mkdtemp(prefix="pool_scratch_driver_")
            atexit.register(shutil.rmtree, _dir, ignore_errors=True)
        _exes[sanitized] = cpu_driver.build(DRIVER, _dir, "pool_scratch_driver" + ("_san" if sanitized else ""),
                                            flags=("-Wno-unknown-pragmas", "-DVHP_SIM", "-O2"), includes=(CSRC,), sanitized=sanitized)
    return _exes[sanitized]


def run(requests, sanitized=False):
    """One list of ints per request line (see the driver's header)."""
    p = subprocess.run([driver(sanitized)], input="\n".join(requests) + "\n", capture_output=True, text=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    rows = [[int(v) for v in line.split()] for line in p.stdout.splitlines()]
    assert len(rows) == len(requests), (len(rows), len(requests))
    return rows


def lines_of_sources(nx, ny, sources):
    """(bound, need, (sx, sy), units with a boundary line, sources) for the sources given, int [n, 2]"""
    flat = " ".join("%d %d" % (int(x), int(y)) for x, y in sources)
    bound, need, sx, sy, units, n = run(["lines %d %d list %d %s" % (nx, ny, len(sources), flat)])[0]
    return bound, need, (sx, sy), units, n
