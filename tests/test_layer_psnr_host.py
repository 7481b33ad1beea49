"""psnr_quantum.h and the tile-split's PSNR exchange (csrc/split.cpp) as a
stand-alone host program under AddressSanitizer and UBSan
(tests/host/test_psnr_quantum.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_psnr_quantum_and_exchange_on_cpu(tmp_path):
    csrc = os.path.join(ROOT, "jp2-bucketeer_amd", "csrc")
    exe = tmp_path / "test_psnr_quantum"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", csrc,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "test_psnr_quantum.cpp"),
                    os.path.join(csrc, "split.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("psnr quantum and exchange: ok")
