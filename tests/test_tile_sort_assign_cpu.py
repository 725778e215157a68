"""The static first round of the tile sort (gaussianip_amd/csrc/tile_sort_assign.h): who sorts which position of tile_order.

tile_sort_assign_check.cpp is a stand-alone program with its own main: it includes the header the kernel includes, is built
here with the host compiler and -fsanitize=address,undefined, and runs as a child process (nothing is preloaded, nothing goes
through Python).  Grid sizes 1, 2, 8, 255, 256 and 304; 0 .. 3 x grid + 5 tiles in each class (the whole cube for the small
grids, every count of one class against the edge counts of the other two for the large ones), plus M beyond four per workgroup
and B beyond two rounds of wave slots.  What it asserts is listed at the top of the program."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gaussianip_amd", "csrc")


def test_static_round_claims_every_position_exactly_once(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "tile_sort_assign_check")
    # the sanitizer runtimes are linked into the program itself, so it needs nothing from the environment it starts in
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + static + ["-I", CSRC, os.path.join(HERE, "tile_sort_assign_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.strip().splitlines()[-1].startswith("ok ")
