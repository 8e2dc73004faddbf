"""The bookkeeping of the timestamps a pool- or latency-sweep launch writes from inside its own kernels (csrc/vhp_stamps.hpp), on the
CPU: tests/stamps_driver.cpp answers one request per line.  The driver is built twice -- plain, and with the address and
undefined-behaviour sanitizers (its stand-in for the device array has exactly the ring's size, and every slot handed out is written
from end to end) --; every case runs through both, each run a process of its own."""
import os
import subprocess

import numpy as np
import pytest

import cpu_driver


@pytest.fixture(scope="module", params=["plain", "san"])
def driver(request, tmp_path_factory):
    san = request.param == "san"
    return cpu_driver.build(os.path.join(cpu_driver.HERE, "stamps_driver.cpp"), str(tmp_path_factory.mktemp("stamps")), "stamps_driver_" + request.param,
                            flags=() if san else ("-O2",), sanitized=san)


def run(exe, requests):
    p = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True, check=False)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    rows = p.stdout.splitlines()
    assert len(rows) == len(requests), rows
    return rows


def f32(x):
    return float(np.float32(x))


def test_slot_sizes(driver):
    # `groups` begin entries (a launch without a pre-kernel: one per workgroup) and `groups` end entries of 16 bytes
    rows = run(driver, ["sizes 1", "sizes 256", "sizes 1024", "sizes 0"])
    assert rows == ["2 32", "512 8192", "2048 32768", "0 0"]
    # the array: slot 0 (the launches with timing off) and the ring's n
    rows = run(driver, ["ring 0 256", "ring 5 256", "offset 0", "offset 1", "offset 5", "fits 1 256", "fits 256 256", "fits 1 512", "fits 257 256", "fits 0 4", "fits 4 0"])
    assert rows[0] == "1 0 256 0 8192"
    assert rows[1] == "1 5 256 0 49152"
    assert rows[2:5] == ["0", "512", "2560"]
    assert rows[5:] == ["1", "1", "0", "0", "0", "0"]


def test_ring_hands_out_wraps_and_runs_dry(driver):
    rows = run(driver, ["ring 3 4", "oldest", "runs", "take", "take", "runs", "take", "take", "take", "oldest", "runs",   # 0..10
                        "release 2", "oldest", "runs", "take", "runs", "take", "take", "runs", "release 3", "runs", "take", "oldest"])   # 11..22
    assert rows[1] == "-1" and rows[2] == "-"
    assert rows[3] == "1 1" and rows[4] == "2 2" and rows[5] == "1:2"
    assert rows[6] == "3 3"
    # full: the caller is told so (and falls back to events) -- never handed slot 1, which nobody has read yet
    assert rows[7] == "-1 3" and rows[8] == "-1 3"
    assert rows[9] == "1" and rows[10] == "1:3"
    # the two oldest back: slot 3 is the oldest now, the next ones wrap to 1 and 2
    assert rows[11] == "1" and rows[12] == "3" and rows[13] == "3:1"
    assert rows[14] == "1 2" and rows[15] == "3:1 1:1"
    assert rows[16] == "2 3" and rows[17] == "-1 3" and rows[18] == "3:1 1:2"
    assert rows[19] == "0" and rows[20] == "-"
    assert rows[21] == "3 1" and rows[22] == "3"


def test_ring_untake_and_resize_only_when_empty(driver):
    rows = run(driver, ["ring 2 8", "take", "untake", "take", "take", "untake", "take", "ring 4 8", "ring 2 8", "release 2", "ring 4 8", "take"])
    assert rows[1] == "1 1" and rows[2] == "0"
    assert rows[3] == "1 1"          # a launch that did not go out leaves no hole: the same slot again
    assert rows[4] == "2 2" and rows[5] == "1" and rows[6] == "2 2"
    assert rows[7].split()[:2] == ["0", "2"]   # slots are out: the ring stays as it is
    assert rows[8].split()[:2] == ["1", "2"]   # (asking for what it is is no change)
    assert rows[10].split()[:2] == ["1", "4"]
    assert rows[11] == "1 1"


def test_ticks_to_ms(driver):
    rows = run(driver, ["ms 100000 100000", "ms 56400 100000", "ms 1 100000", "ms 56400 25000", "ms 123456789 27000", "ms 5 0"])
    # (the rate comes from the device: 100 MHz is what an MI355X reports, nothing the code may assume)
    assert [np.float32(float(r)) for r in rows] == [np.float32(v) for v in (1.0, 0.564, 1e-5, 56400 / 25000, 123456789 / 27000, 0.0)]


TAG = 0x5A17000000000007


def test_reduce_a_slot(driver):
    good = "reduce 100000 1 3 %d 1000:%d 50000:%d 57400:%d 51000:%d" % (TAG, TAG, TAG, TAG, TAG)
    every_group_begins = "reduce 100000 2 2 %d 1200:%d 1000:%d 3000:%d 2000:%d" % (TAG, TAG, TAG, TAG, TAG)
    rows = run(driver, [good, every_group_begins])
    assert rows[0] == "1 %.9g" % f32(56400 / 100000)     # first begin to LAST end
    assert rows[1] == "1 %.9g" % f32(2000 / 100000)      # FIRST begin to last end
    old = TAG - 1
    rows = run(driver, [
        # one end entry still carries an older launch's tag: the launch has not finished -- whether the stale clock is larger or smaller
        "reduce 100000 1 3 %d 1000:%d 50000:%d 99999:%d 51000:%d" % (TAG, TAG, TAG, old, TAG),
        "reduce 100000 1 3 %d 1000:%d 50000:%d 10:%d 51000:%d" % (TAG, TAG, TAG, old, TAG),
        # the begin entry missing (never written: zero, or an older launch's)
        "reduce 100000 1 3 %d 0:0 50000:%d 57400:%d 51000:%d" % (TAG, TAG, TAG, TAG),
        "reduce 100000 1 3 %d 900:%d 50000:%d 57400:%d 51000:%d" % (TAG, old, TAG, TAG, TAG),
        "reduce 100000 2 2 %d 1200:%d 1000:%d 3000:%d 2000:%d" % (TAG, TAG, old, TAG, TAG),
        # the last end before the first begin
        "reduce 100000 1 2 %d 5000:%d 4000:%d 4999:%d" % (TAG, TAG, TAG, TAG),
        # no clock rate, no entries
        "reduce 0 1 3 %d 1000:%d 50000:%d 57400:%d 51000:%d" % (TAG, TAG, TAG, TAG, TAG),
        "reduce 100000 0 3 %d 50000:%d 57400:%d 51000:%d" % (TAG, TAG, TAG, TAG),
        # end == begin is a time (zero), not a failure
        "reduce 100000 1 1 %d 7:%d 7:%d" % (TAG, TAG, TAG),
    ])
    assert [r.split()[0] for r in rows] == ["0"] * 8 + ["1"]
    assert rows[8] == "1 0"


def test_timing_on_one_slot_serves_collect_and_last(driver):
    # three launches, a ring of four: all stamped; collect reports each once, and what vhp_last_elapsed_ms says afterwards -- the slot
    # has gone back to the ring -- is the last of them, the same float
    row = run(driver, ["timed 4 256 100000 3"])[0]
    launches, collect, last, again = [s.strip() for s in row.split("|")]
    assert launches.split() == ["s1", "s2", "s3"]
    times = collect.split()[1:]
    want = "1:%.9g" % f32((500 + 255) / 100000)
    assert times == [want] * 3
    assert last == "last 3 %s" % want[2:]          # (3: Last::kRead)
    assert again == "collect2 0 live 0"
    # five launches, a ring of two: two stamped, the rest by events -- signalled, not a slot that is still out; the last launch was
    # timed by events, and so is what vhp_last_elapsed_ms reports (1: Last::kEvents)
    row = run(driver, ["timed 2 9 100000 5"])[0]
    launches, collect, last, again = [s.strip() for s in row.split("|")]
    assert launches.split() == ["s1", "s2", "ev", "ev", "ev"]
    assert collect.split()[1:] == ["1:%.9g" % f32(508 / 100000)] * 2
    assert last == "last 1 -1"
    assert again == "collect2 0 live 0"
    # another clock rate
    row = run(driver, ["timed 1 1 25000 1"])[0]
    assert row.split("|")[1].split()[1:] == ["1:%.9g" % f32(500 / 25000)]
