"""A DWT level whose rows do not fit in LDS is lifted in column chunks
(csrc/dwt_chunk.h: staged and kept columns, output places, chunk count).  The
geometry has no HIP in it: tests/host/test_dwt_chunk.cpp checks it on the CPU
under AddressSanitizer / UBSan, as its own process, for every row width up to
20000, and lifts random rows chunk by chunk against whole-row lifting, bit for
bit (-ffp-contract=off, as the library is built)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dwt_chunk_on_cpu(tmp_path):
    csrc = os.path.join(ROOT, "jp2-bucketeer_amd", "csrc")
    exe = tmp_path / "test_dwt_chunk"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", csrc,
                    os.path.join(ROOT, "tests", "host", "test_dwt_chunk.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("DWT CHUNK OK")
