"""The crafted Deflate corpus (tests/inflate_cases.py) on the CPU: its writer
and model are pinned to zlib, every stream where the two part is listed with
its reason, the census of k_inflate's paths is complete but for the cells
listed with a reason, and the pins file is what the module measures today.
The streams of the suites that came before the corpus (zlib's and libtiff's
own choices) go through the same model, so that DESIGN.md can say which paths
those suites ever reached.  The kernel itself runs on these streams in
test_inflate_host.py (one lane, under AddressSanitizer) and in
test_gpu_inflate_cases.py."""
import json
import zlib

import imaging as im
import inflate_cases as fc

ROWS = fc.measured()


def test_kernel_constants_are_found_in_the_source():
    k = fc.kernel_constants()
    assert set(k) == {"kInfLB", "kInfDB", "JP2HIP_INF_LANES", "kInChunkWords", "kLinkDoublings", "kLinkChunk"}
    assert all(isinstance(v, int) and v > 0 for v in k.values())
    # what the families are built on: 64 bit offsets a window, 1 KiB a ring refill, codes up to 15 bits walk
    assert k["JP2HIP_INF_LANES"] == 64 and k["kInChunkWords"] * 4 == 1024
    assert k["kInfLB"] < 13 and k["kInfDB"] < 10 and k["kLinkChunk"] == 4096


# ---- the writer and the model against zlib ---------------------------------
def divergences() -> dict:
    """{stream: reason}: every stream of the corpus that the model (and the
    product) accepts and zlib.decompress refuses."""
    out = {}
    for name in ROWS:
        if name.startswith("ends_") and name not in ("ends_wrong_adler32", "ends_no_trailer",
                                                     "ends_data_after_final_block", "ends_exactly_at_final_eob",
                                                     "ends_one_bit_literals_exact",
                                                     "ends_block_ends_at_cap_then_empty_final"):
            out[name] = "the strip is full before the final block ends, and rubbish follows: data after a full " \
                        "strip is not read (libtiff stops there too)"
        if name.startswith("align_1024_") or name.startswith("align_2048_"):
            out[name] = "no Adler-32 trailer, so that the end-of-block code lies in the stream's last byte"
    out["stored_cut_by_cap_then_rubbish"] = out["ends_in_a_literal"]
    for name in ("ends_exactly_at_final_eob", "ends_one_bit_literals_exact",
                 "ends_block_ends_at_cap_then_empty_final"):
        out[name] = "rubbish where the Adler-32 should be: the trailer is not read"
    out["ends_wrong_adler32"] = "Adler-32 is not checked"
    out["ends_no_trailer"] = "a missing trailer is not noticed: nothing is read after the final block"
    out["tables_one_distance_code_incomplete_litlen"] = "an incomplete literal/length code is accepted as long as " \
                                                        "its unused codes never occur"
    out["errors_litlen_unused_code_good"] = out["tables_one_distance_code_incomplete_litlen"]
    out["tables_incomplete_distance_code"] = "an incomplete distance code other than the single 1-bit one is " \
                                             "accepted as long as its unused codes never occur"
    out["tables_incomplete_code_length_code"] = "an incomplete code-length code is accepted as long as its unused " \
                                                "codes never occur"
    return out


def zlib_says(stream: bytes, cap: int):
    """(what zlib.decompress makes of the whole stream, what a decompressobj
    gives when asked for cap bytes); None where zlib raises."""
    try:
        whole = zlib.decompress(stream)
    except zlib.error:
        whole = None
    try:
        first = zlib.decompressobj().decompress(stream, cap)
    except zlib.error:
        first = None
    return whole, first


def test_model_agrees_with_zlib_but_for_the_listed_streams():
    listed, seen = divergences(), set()
    assert all(len(r) > 20 for r in listed.values()) and set(listed) <= set(ROWS)
    for name, (res, cen, stream, cap, head) in ROWS.items():
        whole, first = zlib_says(stream, cap)
        ok = isinstance(res, bytes)
        if whole is not None and len(whole) >= cap:
            # zlib accepts it and it fills the strip: refusing it or decoding it differently is a bug
            assert ok and res == whole[:cap], name
        elif whole is not None:
            assert not ok and res.reason == "short_output", name
        elif ok:
            assert name in listed, f"{name}: the model accepts what zlib refuses, and nobody listed it"
            seen.add(name)
        if ok and first is not None and len(first) == cap:
            assert res == first, name          # the cut at cap against zlib's own first cap bytes
        if ok:
            assert len(res) == cap
    assert seen == set(listed), f"listed, yet zlib agrees: {sorted(set(listed) - seen)}"
    # the listed streams are still checked byte for byte wherever zlib decodes that far
    checked = [n for n in listed if zlib_says(ROWS[n][2], ROWS[n][3])[1] is not None]
    # (not the incomplete codes, which zlib refuses at the table, nor a bad trailer right behind the last byte)
    assert set(listed) - set(checked) == {
        "tables_one_distance_code_incomplete_litlen", "errors_litlen_unused_code_good",
        "tables_incomplete_distance_code", "tables_incomplete_code_length_code", "ends_exactly_at_final_eob",
        "ends_wrong_adler32", "ends_one_bit_literals_exact", "ends_block_ends_at_cap_then_empty_final"}


def test_every_error_stream_is_refused_for_its_own_reason_and_its_twin_is_good():
    doors = set()
    for name, bad, good in fc.error_pairs():
        res = ROWS[name][0]
        assert isinstance(res, fc.Corrupt), name
        doors.add(res.reason)
        assert name[len("errors_"):].startswith(res.reason) or name in (
            "errors_dist_all_zero_table_match", "errors_no_eob_code_ncode_4"), (name, res.reason)
        assert isinstance(ROWS[name + "_good"][0], bytes)
        if name + "_good" not in divergences():
            assert zlib.decompress(good.streams[1]) == ROWS[name + "_good"][0]
        assert bad.streams[0] == good.streams[0] and bad.cap == good.cap <= 4096
    assert doors == set(fc.DOORS) - {"dist_ge_30_check"}


def test_writer_reproduces_the_fixed_block_writer():
    toks = im.crafted_match_tokens(7)[:900]
    assert fc.deflate_stream([fc.fixed(toks)]) == im.deflate_tokens(toks)[0]


# ---- census ----------------------------------------------------------------
def unreachable_cells() -> dict:
    """{cell: reason}: the only way to leave a cell of inflate_cases.CELLS out of the corpus."""
    return {
        "err_dist_ge_30_check": "`if (dc >= 30u) return false` cannot fire: a dynamic block has ndist <= 30 (checked "
                                "before the tables are built) and the fixed block's distance table is built from 30 "
                                "lengths, so the 5-bit codes 30 and 31 have no table entry and leave through the "
                                "unused-distance-code door (cells err_dist_code_30 / _31) before this line",
    }


def test_corpus_reaches_every_cell_but_the_listed_ones():
    tot = fc.totals()
    assert set(tot) == set(fc.CELLS) and len(set(fc.CELLS)) == len(fc.CELLS)
    unreachable = unreachable_cells()
    assert set(unreachable) <= set(tot) and all(len(r) > 40 for r in unreachable.values())
    missed = [k for k, v in tot.items() if not v and k not in unreachable]
    assert not missed, missed
    reached = [k for k in unreachable if tot[k]]
    assert not reached, f"listed as unreachable, yet reached: {reached}"


def test_phase_family_puts_every_match_part_at_every_lane():
    """What the family is for, stated on the streams themselves: over n = 0..127
    the length code of the long match starts at every bit offset of a window."""
    starts = {}
    for n in range(128):
        cen = ROWS[f"phase_{n:03d}"][1]
        for part in ("lenx", "dcode", "distx"):
            for lane in ("0", "63", "mid"):
                starts[(part, lane)] = starts.get((part, lane), 0) + cen.get(f"{part}_lane_{lane}", 0)
        assert cen["dist_walk_15"] >= 1 and cen["blk_stored"] == 1 and cen["blk_dynamic"] == 1
    assert all(v >= 2 for v in starts.values()), starts
    fired = [sum(ROWS[f"phase_{n:03d}"][1].get(f"refill{i}_fired", 0) for n in range(128)) for i in (1, 2, 3)]
    assert min(fired) >= 4, fired


def test_link_chains_are_deep_and_bounded():
    deepest = max(cen.get("max_link_depth", 0) for _, cen, *_ in ROWS.values())
    assert 32 < deepest <= fc.LINK_DEPTH_BOUND
    assert ROWS["links_dist1_len3_x8000"][1]["max_link_depth"] == 8000
    assert ROWS["links_dist1_len3_x33"][1]["max_link_depth"] == 33
    assert ROWS["links_dist1_len3_x32"][1]["max_link_depth"] == 32
    assert "links_left_after_doublings" not in ROWS["links_dist1_len3_x32"][1] or \
        ROWS["links_dist1_len3_x32"][1]["max_link_depth"] >> fc.kernel_constants()["kLinkDoublings"] == 1


def test_strips_are_small_and_start_everywhere():
    big = [f for f in fc.valid_files() if f.cap > 65536]
    assert not big
    assert {h for f in fc.align_files()[:1] for h in f.heads()} == set(range(16))
    assert sum(1 for f in fc.valid_files() if f.compression == 32946) >= len(fc.FAMILIES) - 2
    assert len([n for n in ROWS if n.startswith("random_")]) == 200


def test_pins_are_what_the_module_measures():
    with open(fc.PINS) as f:
        text = f.read()
    assert len(text) < 100_000
    assert json.loads(text) == json.loads(fc.pins_text()), "run `python tests/inflate_cases.py` and review the diff"


# ---- the streams of the suites that came before ----------------------------
def earlier_suite_files() -> dict:
    """The Deflate TIFFs of test_gpu_parity, test_gpu_pixel_formats,
    test_gpu_ingest_streams and test_split, built the way those tests build them."""
    import ingest_stream_cases as isc
    import pixel_format_cases as pf
    out = {}
    rgb, g16 = im.synth_rgb8(301, 517, seed=9), im.synth_u16(301, 517, comps=1, seed=9)
    out["parity_strips_rgb8"] = im.tiff_bytes_compressed(rgb, "tiff_adobe_deflate", rows_per_strip=24)
    out["parity_strips_gray16_pred"] = im.tiff_bytes_compressed(g16, "tiff_adobe_deflate", predictor=True,
                                                                rows_per_strip=24)
    out["parity_strips_rgb8_pred_32946"] = im.tiff_bytes_compressed(rgb, "tiff_deflate", predictor=True,
                                                                    rows_per_strip=24)
    out["parity_tiles_rgb8"] = im.tiled_tiff_bytes(im.synth_rgb8(301, 517, seed=5), tile=(64, 48), deflate=True)
    out["parity_tiles_rgb16_planar"] = im.tiled_tiff_bytes(im.synth_u16(301, 517, comps=3, seed=5), tile=(64, 48),
                                                           deflate=True, planar=True)
    out["parity_corrupt_tests_good_file"] = im.tiff_bytes_compressed(im.synth_rgb8(64, 64, seed=1),
                                                                     "tiff_adobe_deflate", rows_per_strip=32)
    for c in pf.decoder_cases():
        if c["kw"].get("codec") == "deflate":
            out["pixel_formats_" + c["id"]] = pf.build(c)[0]
    for c in isc.LAYOUT_CASES:
        if c["codec"] == "deflate":
            out["ingest_" + c["id"]] = isc.layout_build(c)[0]
    img = im.synth_rgb8(300, 170, seed=2)
    out["split_tiles_planar"] = im.tiled_tiff_bytes(img, tile=(32, 48), planar=True, deflate=True)
    rgb = im.synth_rgb8(1300, 700, seed=21)
    out["split_strips_pillow"] = im.tiff_bytes_compressed(rgb, "tiff_adobe_deflate", rows_per_strip=40)
    out["split_tiles_planar_big"] = im.tiled_tiff_bytes(rgb, tile=(64, 48), planar=True, deflate=True)
    return out


def earlier_suite_totals(sample=3):
    tot, n = dict.fromkeys(fc.CELLS, 0), 0
    for name, tif in earlier_suite_files().items():
        units = fc.tiff_units(tif)
        assert units, name
        # (`sample` units of each file, spread over it: the model is plain Python)
        for stream, cap, head in (units[::max(1, len(units) // sample)][:sample] if sample else units):
            res, cen = fc.inflate_model(stream, cap, head)
            assert isinstance(res, bytes) and res == zlib.decompress(stream)[:cap], name
            n += 1
            for k, v in cen.items():
                if k in tot:
                    tot[k] += v
    # the one crafted case from before: two strips of one fixed block each
    for seed in (7, 8):
        stream, raw = im.deflate_tokens(im.crafted_match_tokens(seed))
        res, cen = fc.inflate_model(stream, len(raw))
        assert res == raw
        n += 1
        for k, v in cen.items():
            if k in tot:
                tot[k] += v
    return tot, n


# What the suites before this corpus never reached, over all 1502 of their streams (measured once with
# earlier_suite_totals(sample=0), a minute of plain Python; the test below takes three units of each file).
# DESIGN.md 2, "Deflate corpus", has the table.  They did run the long-code walk: 13 and 14 bits, on noisy
# 16-bit samples -- not 15 bits, not at the distance table past 11 bits, and no error door but three.
NEVER_BEFORE = (
    "pair_stored_stored", "pair_stored_fixed", "pair_stored_dynamic", "pair_fixed_stored", "pair_fixed_fixed",
    "pair_fixed_dynamic", "pair_dynamic_stored", "pair_dynamic_fixed", "blk_final_empty",
    "blk_nonfinal_ends_at_cap", "stored_len_0", "stored_len_65535", "stored_cut_by_cap", "stored_aligned",
    "stored_pad_1", "stored_pad_2", "stored_pad_3", "stored_pad_4", "stored_pad_6", "stored_pad_7",
    "stored_skip_in_ring", "stored_skip_restart", "stored_after_eob_at_bit7", "nlen_257", "ndist_1", "ncode_4",
    "ncode_19", "cl_repeat_crosses_boundary", "dist_table_all_zero", "dist_table_one_1bit",
    "dist_table_incomplete_other", "litlen_incomplete", "ll_walk_15", "run_64", "full_in_literal",
    "full_in_long_literal", "dist_walk_12", "dist_walk_13", "dist_walk_14", "dist_walk_15", "dist_eq_pos",
    "match_cut_by_cap", "match_at_cap", "ring_exact_1024", "ring_exact_2048", "ring_over_1", "ring_over_2",
    "ring_over_3")


def test_which_cells_the_earlier_suites_reached():
    tot, n = earlier_suite_totals()
    assert n > 60
    print(json.dumps({"streams": n, "reached": sum(1 for v in tot.values() if v), "cells": len(tot),
                      "empty": [k for k, v in tot.items() if not v]}))
    for cell in NEVER_BEFORE:
        assert tot[cell] == 0, cell
        assert fc.totals()[cell] > 0, cell
    # ... and what they did reach, so that the table's other column is measured too
    for cell in ("blk_stored", "blk_fixed", "blk_dynamic", "ll_fast", "ll_walk_13", "ll_walk_14", "refill1_fired",
                 "refill2_fired", "refill3_fired", "dist_32768", "overlap_dist_lt_64", "links_depth_gt_32"):
        assert tot[cell] > 0, cell
