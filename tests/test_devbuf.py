"""The owning buffer behind every device scratch and state array (csrc/vhp_devbuf.hpp), on the CPU: tests/devbuf_driver.cpp runs it
over an allocator that counts live blocks, records every size it is asked for and fails on request.  The driver is built twice --
plain, and with the address and undefined-behaviour sanitizers (it writes every block from end to end) --; every scenario runs through
both, each run a process of its own that exits 0 only with no block live."""
import os
import subprocess

import pytest

import cpu_driver

FAILED = 7   # the driver's allocator's error


@pytest.fixture(scope="module", params=["plain", "san"])
def driver(request, tmp_path_factory):
    san = request.param == "san"
    return cpu_driver.build(os.path.join(cpu_driver.HERE, "devbuf_driver.cpp"), str(tmp_path_factory.mktemp("devbuf")), "devbuf_driver_" + request.param,
                            flags=() if san else ("-O2",), sanitized=san)


def run(exe, requests):
    """Per request: (grow's return value, the four slots, the sizes asked of the allocator, frees, live blocks)."""
    p = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])   # (0: every request well-formed and no block live at exit)
    rows = []
    for line in p.stdout.splitlines():
        f = line.split()
        slots = [None if s == "-" else tuple(int(v) for v in s.split(":")) for s in f[1:5]]
        rows.append((int(f[0]), slots, [] if f[5] == "-" else [int(v) for v in f[5].split(",")], int(f[6]), int(f[7])))
    assert len(rows) == len(requests)
    return rows


EMPTY = (0, 0)


def test_grow_only(driver):
    rows = run(driver, ["new 0", "grow 0 100", "grow 0 100", "grow 0 40", "grow 0 1", "grow 0 101", "grow 0 4096", "grow 0 4095"])
    assert rows[0] == (0, [EMPTY, None, None, None], [], 0, 0)
    assert rows[1] == (0, [(1, 100), None, None, None], [100], 0, 1)      # the first request: one allocation, nothing to free
    for r in rows[2:5]:                                                    # within capacity: no allocator call at all
        assert r == (0, [(1, 100), None, None, None], [], 0, 1)
    assert rows[5] == (0, [(1, 101), None, None, None], [101], 1, 1)      # one byte more: exactly one free, one allocation of that size
    assert rows[6] == (0, [(1, 4096), None, None, None], [4096], 1, 1)
    assert rows[7] == (0, [(1, 4096), None, None, None], [], 0, 1)


def test_zero_bytes_never_allocates(driver):
    rows = run(driver, ["new 0", "grow 0 0", "grow 0 8", "grow 0 0", "reset 0", "grow 0 0"])
    assert rows[1] == (0, [EMPTY, None, None, None], [], 0, 0)
    assert rows[3] == (0, [(1, 8), None, None, None], [], 0, 1)
    assert rows[5] == (0, [EMPTY, None, None, None], [], 0, 0)


def test_failed_grow_leaves_an_empty_buffer(driver):
    # the planner's pivot list: a solve with many iterations, a larger one whose allocation fails, then a SMALLER one -- which must
    # allocate, not find the old size beside a null pointer
    rows = run(driver, ["new 0", "grow 0 168", "fail 1", "grow 0 4000", "grow 0 48", "grow 0 168", "fail 1", "grow 0 8", "new 1", "fail 1",
                        "grow 1 16", "grow 1 16"])
    assert rows[1] == (0, [(1, 168), None, None, None], [168], 0, 1)
    assert rows[3] == (FAILED, [EMPTY, None, None, None], [4000], 1, 0)   # the old block freed, the new one refused: null and 0 bytes
    assert rows[4] == (0, [(1, 48), None, None, None], [48], 0, 1)        # the smaller request allocates again
    assert rows[5] == (0, [(1, 168), None, None, None], [168], 1, 1)
    assert rows[7] == (0, [(1, 168), None, None, None], [], 0, 1)         # (within capacity nothing is asked for, so nothing can fail)
    assert rows[10] == (FAILED, [(1, 168), EMPTY, None, None], [16], 0, 1)   # a first allocation that fails
    assert rows[11] == (0, [(1, 168), (1, 16), None, None], [16], 0, 2)


def test_moves_leave_the_source_empty_and_free_nothing(driver):
    rows = run(driver, ["new 0", "grow 0 64", "movec 0 1", "grow 0 8", "new 2", "movea 1 2", "grow 1 0", "delete 1", "movea 0 2", "delete 0"])
    assert rows[2] == (0, [EMPTY, (1, 64), None, None], [], 0, 1)          # move construction
    assert rows[3] == (0, [(1, 8), (1, 64), None, None], [8], 0, 2)        # (the source is a buffer like any other afterwards)
    assert rows[5] == (0, [(1, 8), EMPTY, (1, 64), None], [], 0, 2)        # move assignment into an empty buffer
    assert rows[7] == (0, [(1, 8), None, (1, 64), None], [], 0, 2)         # the moved-from buffer's destructor frees nothing
    assert rows[8] == (0, [EMPTY, None, (1, 8), None], [], 1, 1)           # ... into a buffer that holds a block: that block goes, once
    assert rows[9] == (0, [None, None, (1, 8), None], [], 0, 1)


def test_reset_and_destructor_free_once(driver):
    rows = run(driver, ["new 0", "grow 0 32", "reset 0", "reset 0", "delete 0", "new 1", "grow 1 32", "delete 1", "new 2", "delete 2"])
    assert rows[2] == (0, [EMPTY, None, None, None], [], 1, 0)
    assert rows[3] == (0, [EMPTY, None, None, None], [], 0, 0)             # a second reset, and the destructor after it: nothing more
    assert rows[4] == (0, [None, None, None, None], [], 0, 0)
    assert rows[7] == (0, [None, None, None, None], [], 1, 0)              # the destructor of a buffer that holds a block
    assert rows[9] == (0, [None, None, None, None], [], 0, 0)              # ... and of one that never did


def test_adopt_is_freed_once(driver):
    rows = run(driver, ["new 0", "adopt 0 24", "grow 0 24", "grow 0 25", "adopt 0 10", "delete 0", "new 1", "adopt 1 5"])
    assert rows[1] == (0, [(1, 24), None, None, None], [24], 0, 1)         # (the allocation is the driver's own)
    assert rows[2] == (0, [(1, 24), None, None, None], [], 0, 1)           # an adopted block is capacity like any other
    assert rows[3] == (0, [(1, 25), None, None, None], [25], 1, 1)
    assert rows[4] == (0, [(1, 10), None, None, None], [10], 1, 1)         # adopting over a block frees that block
    assert rows[5] == (0, [None, None, None, None], [], 1, 0)
    assert rows[7] == (0, [None, (1, 5), None, None], [5], 0, 1)           # (left to the end of the run: the exit code says it was freed)
