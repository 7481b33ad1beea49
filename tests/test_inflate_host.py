"""k_inflate (csrc/inflate_kernels.h, the text unpack.hip includes) compiled for the host -- a one-lane wave --
and run under AddressSanitizer:
zlib streams of every level at every byte alignment decode exactly, and
truncated or reserved-block streams report a corrupt strip.  The GPU tests
(test_gpu_parity.py) run the same kernel on the device; this one runs on CPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(__file__)
CSRC = os.path.join(HERE, "..", "jp2-bucketeer_amd", "csrc")
CLANG = "/opt/rocm/llvm/bin/clang++"

# the kernel's arguments and the two kernels, as unpack.hip sees them
KERNEL_TEXT = 'namespace jp2hip {\n#include "unpack_args.h"\n#include "inflate_kernels.h"\n}\n'


@pytest.mark.skipif(not os.path.exists(CLANG) or not os.path.exists("/usr/include/zlib.h"),
                    reason="needs ROCm clang++ and zlib headers")
def test_inflate_host_build(tmp_path):
    main = open(os.path.join(HERE, "host", "inflate_main.cpp")).read()
    shims, rest = main.split("// [[MAIN]]")
    src = tmp_path / "inflate_host.cpp"
    src.write_text(shims + KERNEL_TEXT + rest)
    exe = tmp_path / "inflate_host"
    subprocess.run([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address", "-I", CSRC, str(src), "-o", str(exe), "-lz"],
                   check=True, capture_output=True, timeout=240)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("OK")
