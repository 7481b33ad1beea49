"""The source-layout module (csrc/source_layout.cpp: the TIFF parser, the
unit grid, the band walk -- what stands between a strip table and a kernel
reading outside its buffer) has no HIP in it: compiled with g++ and run on
the CPU, under AddressSanitizer/UBSan, by tests/host/test_source_layout.cpp."""
import os
import subprocess

import numpy as np

import imaging as im
import metadata_fixtures as mf
import pixel_format_cases as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parser_fixtures():
    """Small TIFFs of every form the parser walks differently."""
    rgb = im.synth_rgb8(11, 9, seed=3)
    return {
        "rgb8_strips": im.tiff_bytes(rgb, rows_per_strip=4),
        "bigtiff": im.bigtiff_bytes(rgb, rows_per_strip=4),
        "tiled_deflate_planar": im.tiled_tiff_bytes(im.synth_rgb8(20, 40, seed=4), tile=(16, 16), planar=True,
                                                    deflate=True),
        "palette4_lzw_be": pf.make_tiff(pf.indices(11, 9, 4, 5), 4, pf.PALETTE, colormap=pf.random_colormap(4, 6),
                                        big_endian=True, rows_per_strip=4, codec="lzw"),
        "bilevel_wiz_lsb": pf.make_tiff(pf.indices(11, 21, 1, 7), 1, pf.WHITE_IS_ZERO, fill_order=2, rows_per_strip=4),
        "icc_and_resolution": mf.tag_source(im.tiff_bytes(np.ascontiguousarray(rgb[:5]), rows_per_strip=4),
                                            icc=mf.icc_profile(), xres=(300, 1), yres=(300, 1), unit=2),
    }


def test_source_layout_on_cpu(tmp_path):
    csrc = os.path.join(ROOT, "jp2-bucketeer_amd", "csrc")
    exe = tmp_path / "test_source_layout"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-Wall", "-Wextra", "-Werror",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "test_source_layout.cpp"),
                    os.path.join(csrc, "source_layout.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    paths = []
    for name, tif in parser_fixtures().items():
        assert len(tif) < 4096, (name, len(tif))  # every prefix is parsed: keep them small
        paths.append(str(tmp_path / (name + ".tif")))
        with open(paths[-1], "wb") as f:
            f.write(tif)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0")
    r = subprocess.run([str(exe)] + paths, capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("SOURCE LAYOUT OK (%d files)" % len(paths))
