"""Builds the tests' stand-alone CPU drivers (tests/*_driver.cpp: host-only headers of csrc/ behind a main of their own) with the host
C++ compiler, plain or under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "visibility-heuristic-path-planner_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def compiler():
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (set CXX)"
    return cxx


def build(source, out_dir, name, flags=(), includes=(CSRC,), sanitized=False):
    """The executable out_dir/name from `source`: -std=c++17 -Wall -Werror, the caller's flags, then SANITIZE if asked for (last, so
    that its -O1 is the level of a sanitized build whatever the flags say)."""
    exe = os.path.join(out_dir, name)
    subprocess.check_call([compiler(), "-std=c++17", "-Wall", "-Werror", *flags, *(SANITIZE if sanitized else ()),
                           *[a for d in includes for a in ("-I", d)], "-o", exe, source])
    return exe
