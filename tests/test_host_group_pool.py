"""The two host algorithms behind a tile-split and the output buffers
(csrc/host_group.h, csrc/pinned_pool.cpp): no HIP in them, so they are
compiled with g++ into stand-alone programs (tests/host/) and run on the CPU
under sanitizers.  A hang of the group is a failure here (the runs' timeout),
not a stuck suite."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jp2-bucketeer_amd", "csrc")


def _build_and_run(tmp_path, name, sanitize, sources, expect):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitize, "-Wall", "-Wextra",
                    "-Werror", "-I", CSRC, *sources, "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith(expect)


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_host_group_on_cpu(tmp_path, sanitize):
    """Sums over worlds 1, 2, 4 and 7 through 2 000 back-to-back exchanges of
    changing length, and the abort rules: ranks out of step, n < 0, abort()
    with ranks waiting, reduce after an abort, abort() after the last exchange."""
    _build_and_run(tmp_path, "test_host_group", sanitize, [os.path.join(ROOT, "tests", "host", "test_host_group.cpp")],
                   "HOST GROUP OK")


def test_pinned_pool_on_cpu(tmp_path):
    """The pool's arithmetic with counting malloc / free as the allocator:
    reuse window, best fit, new capacity, idle cap and eviction order."""
    _build_and_run(tmp_path, "test_pinned_pool", "address,undefined",
                   [os.path.join(ROOT, "tests", "host", "test_pinned_pool.cpp"), os.path.join(CSRC, "pinned_pool.cpp")],
                   "PINNED POOL OK")
