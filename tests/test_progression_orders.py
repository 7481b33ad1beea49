"""Progression orders on the CPU (tests/progression_cases.py):

* the expected-file construction -- the oracle's RPCL file re-sequenced --
  against an independent tile-part walk and OpenJPEG, for every order: this
  pins what tests/test_gpu_progression_orders.py compares the GPU's files to;
* jp2hip_packet_sequence, the function libjp2hip's tier-2 tables take the
  order from, against the key sort of the helper over a seeded sweep of small
  geometries; the tables built from it, over the same sweep, in a stand-alone
  program under AddressSanitizer / UBSan;
* the recipes build_plan refuses, by the field the message names.
"""
import os
import subprocess

import numpy as np
import pytest

import imaging as im
import jp2hip
import progression_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = range(5)


def _decode(data):
    """Pixels by OpenJPEG -- opj_decompress, else Pillow's -- or None where
    neither is present."""
    if im.opj("opj_decompress") is not None:
        return im.decode_opj(data, ".j2k")
    try:
        import PIL.features
        if not PIL.features.check_codec("jpg_2000"):
            return None
    except ImportError:
        return None
    return im.decode_pillow(data)


@pytest.fixture(scope="module")
def rpcl_files():
    """name -> (pixels, the jp2hip recipe without an order, the oracle's RPCL
    file): the three geometries with one tile-part per tile, and the RGB one
    with a tile-part per resolution in flush stripes."""
    out = {}
    for name in pc.GEOMETRIES:
        img = pc.image(name)
        out[name] = (img, pc.overrides(name, pc.RPCL))
    out["rgb_300_tpr"] = (pc.image("rgb_300"), pc.overrides("rgb_300", pc.RPCL, tparts_r=1, flush_period=128))
    return {k: (img, ov, pc.oracle_rpcl(img, jp2hip.recipe(jp2hip.LOSSLESS, **ov))) for k, (img, ov) in out.items()}


CASES = [(n, o) for n in list(pc.GEOMETRIES) + ["rgb_300_tpr"] for o in ORDERS
         if n != "rgb_300_tpr" or o in (pc.RLCP, pc.RPCL)]


@pytest.mark.parametrize("name,order", CASES, ids=[f"{n}-{pc.NAMES[o]}" for n, o in CASES])
def test_resequenced_oracle_file_is_a_code_stream_of_that_order(rpcl_files, name, order):
    img, _, rpcl = rpcl_files[name]
    got = pc.resequence(rpcl, order)
    if order == pc.RPCL:
        assert pc.first_difference(got, rpcl) is None, "the RPCL round trip is not the oracle's file"
    else:
        assert got != rpcl
    assert im.main_header_segments(got)["ff52"][5] == order
    im.tile_part_walk(got, 1)
    px = _decode(got)
    if px is not None:
        assert np.array_equal(px.reshape(img.shape), img)


def test_without_plt_is_what_the_oracle_writes(rpcl_files):
    """without_plt (the GPU suite's plt = 0 expectation) on the RPCL file is
    the oracle's own plt = 0 file.  (Without the COM markers: Kdu-Layer-Info
    counts the tile-part headers into each layer's bytes, PLT included.)"""
    img, ov, _ = rpcl_files["rgb_t128"]
    ov = dict(ov, comment=0)
    rpcl = pc.oracle_rpcl(img, jp2hip.recipe(jp2hip.LOSSLESS, **ov))
    want = pc.oracle_rpcl(img, jp2hip.recipe(jp2hip.LOSSLESS, **dict(ov, plt=0)))
    assert pc.first_difference(pc.without_plt(rpcl), want) is None


# ---- jp2hip_packet_sequence against the key sort --------------------------------

def _sweep(n=300, seed=20261020):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        levels = int(rng.integers(0, 6))
        unit = 1 << levels
        pick = lambda: int(rng.choice([16, 32, 48, 64, 96, 128, 256]))
        tw, th = pick(), pick()
        if rng.random() < 0.5:
            th = tw
        tw, th = -(-tw // unit) * unit, -(-th // unit) * unit
        # ragged edges; a last tile of 1..3 samples has empty low resolutions' bands
        w = int(tw * rng.integers(1, 4) - (rng.integers(0, tw) if rng.random() < 0.7 else 0))
        h = int(th * rng.integers(1, 4) - (rng.integers(0, th) if rng.random() < 0.7 else 0))
        if rng.random() < 0.3:
            w = tw * int(rng.integers(1, 3)) + int(rng.integers(1, 4))
        npre = int(rng.integers(0, 4))
        lo = 1 if levels else 0
        # 2^1 .. 2^9: from many precincts per tile to precincts larger than the tile
        pw = [int(rng.integers(max(lo, 1), 10)) for _ in range(npre)]
        ph = [int(rng.integers(max(lo, 1), 10)) for _ in range(npre)]
        out.append(dict(w=max(1, w), h=max(1, h), nc=int(rng.integers(1, 5)),
                        recipe=dict(levels=levels, layers=int(rng.integers(1, 5)), tile_w=tw, tile_h=th,
                                    nprecincts=npre, prec_w_log2=pw, prec_h_log2=ph, tparts_r=0)))
    return out


def test_packet_sequence_is_the_key_sort_on_a_seeded_sweep():
    npk = 0
    for case in _sweep():
        for order in ORDERS:
            rc = jp2hip.recipe(jp2hip.LOSSLESS, progression=order, **case["recipe"])
            g = pc.geometry_of_recipe(case["w"], case["h"], case["nc"], rc)
            for t in range(pc.ntiles(g)):
                got = jp2hip.packet_sequence(case["w"], case["h"], case["nc"], 8, rc, t)
                want = pc.tile_sequence(g, t, order)
                assert got == want, (case, pc.NAMES[order], t)
                if order == pc.RPCL:
                    assert got == list(range(len(got))), (case, t)
                npk += len(got)
    assert npk > 100000  # (the sweep is not made of empty tiles)


def test_sequence_tables_under_sanitizers(tmp_path):
    """Every third case of the sweep through packet_sequence and t2_tables in
    a stand-alone program built with AddressSanitizer / UBSan (tests/host/
    test_packet_sequence.cpp): the invariants the tile-part kernels rely on.
    (Most of the test's time is the compile.)"""
    csrc = os.path.join(ROOT, "jp2-bucketeer_amd", "csrc")
    exe = tmp_path / "test_packet_sequence"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-Wall",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host", "test_packet_sequence.cpp"),
                    os.path.join(csrc, "t2.cpp"), os.path.join(csrc, "plan.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    cases = _sweep()[::3]
    with open(tmp_path / "cases.txt", "w") as f:
        for c in cases:
            r = c["recipe"]
            f.write(" ".join(str(v) for v in [c["w"], c["h"], c["nc"], r["levels"], r["layers"], r["tile_w"], r["tile_h"],
                                              r["nprecincts"]] + r["prec_w_log2"] + r["prec_h_log2"]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert r.stdout.strip() == "PACKET SEQUENCE OK (%d cases)" % len(cases)


def test_packet_sequence_refuses_a_tile_outside_the_image():
    rc = jp2hip.recipe(jp2hip.LOSSLESS, progression=pc.LRCP, tparts_r=0)
    with pytest.raises(jp2hip.Jp2hipError, match="tile"):
        jp2hip.packet_sequence(600, 600, 3, 8, rc, 4)
    assert len(jp2hip.packet_sequence(600, 600, 3, 8, rc, 3)) > 0


# ---- refusals -----------------------------------------------------------------

@pytest.mark.parametrize("order", [-1, 5])
def test_progression_outside_0_to_4_is_refused(order):
    rc = jp2hip.recipe(jp2hip.LOSSLESS, progression=order, tparts_r=0)
    with pytest.raises(jp2hip.Jp2hipError, match="progression"):
        jp2hip.packet_sequence(100, 100, 3, 8, rc, 0)


@pytest.mark.parametrize("order", [pc.LRCP, pc.PCRL, pc.CPRL], ids=["LRCP", "PCRL", "CPRL"])
def test_tile_part_per_resolution_needs_a_resolution_major_order(order):
    rc = jp2hip.recipe(jp2hip.LOSSLESS, progression=order, tparts_r=1)
    with pytest.raises(jp2hip.Jp2hipError, match=f"tparts_r.*{pc.NAMES[order]}"):
        jp2hip.packet_sequence(100, 100, 3, 8, rc, 0)


@pytest.mark.parametrize("order", [pc.RLCP, pc.RPCL], ids=["RLCP", "RPCL"])
def test_tile_part_per_resolution_is_accepted_in_resolution_major_orders(order):
    rc = jp2hip.recipe(jp2hip.LOSSLESS, progression=order, tparts_r=1)
    assert len(jp2hip.packet_sequence(100, 100, 3, 8, rc, 0)) == 7 * 3 * 6


def test_order_constants_are_the_cod_values():
    assert (jp2hip.ORDER_LRCP, jp2hip.ORDER_RLCP, jp2hip.ORDER_RPCL, jp2hip.ORDER_PCRL, jp2hip.ORDER_CPRL) == \
        (0, 1, 2, 3, 4)
    assert jp2hip.recipe(jp2hip.LOSSY).progression == jp2hip.ORDER_RPCL
