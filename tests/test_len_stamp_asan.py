"""Tree's length stamp (pepr_amd/csrc/host.hpp: the writers of Tree::len, what a replayed scoring plan compares instead of the
lengths) in a stand-alone program compiled with g++ -fsanitize=address,undefined: tests/host_asan/len_stamp_driver.cpp.
Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_length_stamp_under_asan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "len_stamp_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           os.path.join(ROOT, "tests", "host_asan", "len_stamp_driver.cpp"), os.path.join(ROOT, "pepr_amd", "csrc", "host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "checks ok" in r.stdout
