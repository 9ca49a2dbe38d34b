"""The depth-map loader (rtxn_load_png_gray16: host-only C++ over the PNG decoder) under AddressSanitizer + UBSan on damaged depth
PNGs.  tools/san/depth_png_fuzz.cpp is built together with rtx_nerf_amd/csrc/loader.cpp by g++ -fsanitize=address,undefined,
exactly as tests/test_loader_sanitized.py builds its harness, checks that valid gray PNGs of 16 and 8 bits (plain and Adam7, every
row filter) load to the values written, and then loads a few thousand truncated, bit-flipped and re-headed copies.  CPU only: a
stand-alone program, nothing preloaded, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("san") / "depth_png_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rtx_nerf_amd", "csrc"),
           os.path.join(ROOT, "rtx_nerf_amd", "csrc", "loader.cpp"), os.path.join(ROOT, "tools", "san", "depth_png_fuzz.cpp"), "-lz", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "sanitize" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr:
            pytest.skip("this g++ has no sanitizer runtime")
        pytest.fail(r.stderr[-2000:])
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_depth_loader_has_no_sanitizer_report_on_damaged_depth_maps(harness, tmp_path, seed):
    r = subprocess.run([harness, str(tmp_path), "3000", str(seed)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "no sanitizer report" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    accepted = int(r.stdout.split("corrupted loads,")[1].split("accepted")[0])
    assert 150 < accepted < 2850          # the campaign reaches both outcomes: files that still load and files that are refused
