"""k_dwt_l1s loads a chunky pixel with one access (csrc/dwt_fetch.h: 4 bytes
for RGB8, one more than the pixel; 8 for RGB16, two more).  The address, size
and byte-extraction arithmetic has no HIP in it: tests/host/test_dwt_fetch.cpp
runs it on the CPU under AddressSanitizer / UBSan, as its own process, over
sources that are exactly as long as their last strip."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dwt_fetch_on_cpu(tmp_path):
    csrc = os.path.join(ROOT, "jp2-bucketeer_amd", "csrc")
    exe = tmp_path / "test_dwt_fetch"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Wextra", "-Werror", "-I", csrc,
                    os.path.join(ROOT, "tests", "host", "test_dwt_fetch.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("DWT FETCH OK")
