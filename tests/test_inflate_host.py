"""k_inflate and k_inflate_links (csrc/inflate_kernels.h, the text unpack.hip includes) compiled for the host
-- a one-lane wave -- as a stand-alone program and run under AddressSanitizer:
zlib streams of every level at every byte alignment decode exactly, truncated
or reserved-block streams report a corrupt strip, and every stream of the
crafted corpus (tests/inflate_cases.py: the blocks, tables, ends, link chains
and error doors zlib never writes) decodes to the model's bytes or is refused,
whatever the link buffer held before.  This checks the serial logic; what only
64 lanes can get wrong (window refills by lane, ballot ranks, per-lane ring
loads) is run on the device by test_gpu_inflate_cases.py on the same corpus,
next to zlib's own streams in test_gpu_parity.py."""
import os
import struct
import subprocess

import pytest

import inflate_cases as fc

HERE = os.path.dirname(__file__)
CSRC = os.path.join(HERE, "..", "jp2-bucketeer_amd", "csrc")
CLANG = "/opt/rocm/llvm/bin/clang++"

# the kernel's arguments and the two kernels, as unpack.hip sees them
KERNEL_TEXT = 'namespace jp2hip {\n#include "unpack_args.h"\n#include "inflate_kernels.h"\n}\n'

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG) or not os.path.exists("/usr/include/zlib.h"),
                                reason="needs ROCm clang++ and zlib headers")


def build_host_program(folder, csrc=CSRC):
    main = open(os.path.join(HERE, "host", "inflate_main.cpp")).read()
    shims, rest = main.split("// [[MAIN]]")
    src = os.path.join(str(folder), "inflate_host.cpp")
    with open(src, "w") as f:
        f.write(shims + KERNEL_TEXT + rest)
    exe = os.path.join(str(folder), "inflate_host")
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address", "-I", csrc, src, "-o", exe, "-lz"],
                   check=True, capture_output=True, timeout=240)
    return exe


def corpus_records() -> bytes:
    """Every stream of the corpus for the program's second mode (the layout
    is described in host/inflate_main.cpp)."""
    rows = fc.measured()
    out = [b"INFC", struct.pack("<I", len(rows))]
    for name, (res, cen, stream, cap, head) in rows.items():
        bad = not isinstance(res, bytes)
        out.append(struct.pack("<I", len(name)) + name.encode())
        out.append(struct.pack("<IIII", head, cap, int(bad), len(stream)) + stream)
        if not bad:
            assert len(res) == cap
            out.append(res)
    return b"".join(out)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("inflate_host"))


def test_inflate_host_build(host_exe):
    p = subprocess.run([host_exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("OK")


def test_inflate_host_corpus(host_exe, tmp_path):
    path = tmp_path / "corpus.bin"
    path.write_bytes(corpus_records())
    p = subprocess.run([host_exe, str(path)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert p.stdout.strip().endswith("OK") and f"{len(fc.measured())} cases" in p.stdout
