"""Which kernel form lifts each DWT level, on what grid and with how much LDS,
is decided by csrc/dwt_route.h; launch_dwt (dwt.hip) only dispatches on it.
The header has no HIP in it: tests/host/test_dwt_route.cpp checks it on the
CPU under AddressSanitizer / UBSan, as its own process -- a sweep of every
plane width up to 32768 against the invariants of each form, and the pinned
routes of the shapes the GPU cases are laid around.  route() is the same
program's --route, for the tests that lay cases around a threshold
(tests/test_large_tiles.py)."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("level", "W", "H", "threads", "cpt", "gx", "gy", "gz", "lds")


@functools.lru_cache(maxsize=None)
def route_exe():
    """tests/host/test_dwt_route.cpp, built once per session."""
    csrc = os.path.join(ROOT, "jp2-bucketeer_amd", "csrc")
    d = tempfile.mkdtemp(prefix="dwt_route_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "test_dwt_route")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", csrc,
                    os.path.join(ROOT, "tests", "host", "test_dwt_route.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    return exe


def _run(*args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    return subprocess.run([route_exe(), *map(str, args)], capture_output=True, text=True, timeout=300, env=env)


@functools.lru_cache(maxsize=None)
def route(tile_w, tile_h, nc, levels):
    """One tile's launches in order: dicts of form (a DwtForm name) and FIELDS."""
    r = _run("--route", tile_w, tile_h, nc, levels)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        form, *nums = line.split()
        out.append(dict(zip(FIELDS, map(int, nums)), form=form))
    return out


def test_dwt_route_on_cpu():
    r = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().startswith("DWT ROUTE OK")
