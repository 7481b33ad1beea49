"""ctypes binding of libjp2hip (include/jp2hip.h).

The shared library is built in-tree by ``__graft_entry__.build()`` (or
``make -C jp2-bucketeer_amd/csrc``) next to this file.  There is no fallback:
if the library or a gfx950 device is missing, calls raise ``Jp2hipError``.
"""
from __future__ import annotations

import ctypes
import math
import os
from ctypes import (CFUNCTYPE, POINTER, Structure, byref, c_char_p, c_double, c_int, c_int32,
                    c_int64, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JP2HIP_LIBRARY") or os.path.join(HERE, "libjp2hip.so")  # override: experiments only

LOSSY = 0      # Conversion.LOSSY    (Conversion.java:9)
LOSSLESS = 1   # Conversion.LOSSLESS (Conversion.java:9)
FORMAT_J2K, FORMAT_JP2, FORMAT_JPX = 0, 1, 2
# Layout.photometric (JP2HIP_PHOTO_*)
PHOTO_DEFAULT, PHOTO_WHITE_IS_ZERO, PHOTO_PALETTE = 0, 1, 2
# Recipe.progression (JP2HIP_ORDER_*: COD's progression order)
ORDER_LRCP, ORDER_RLCP, ORDER_RPCL, ORDER_PCRL, ORDER_CPRL = 0, 1, 2, 3, 4
# Stats.reused (JP2HIP_REUSED_*, JP2HIP_AFTER_*): what an encode found in place
REUSED_PLAN, REUSED_FRONT_TABLES, REUSED_T2_TABLES, REUSED_STRIPS, AFTER_TRIM, AFTER_FAILURE = 1, 2, 4, 8, 16, 32
# jp2hip_set_source_orientation: off (the default), a TIFF Orientation 1..8, or the file's own tag 274
ORIENT_OFF, ORIENT_TIFF = 0, 9


class Jp2hipError(OSError):
    """Raised for every libjp2hip failure (maps to IOException on the Java side)."""


class Config(Structure):
    _fields_ = [("device", c_int32), ("host_threads", c_int32), ("profile", c_int32),
                ("reserved", c_int32)]


class Recipe(Structure):
    _fields_ = [("levels", c_int32), ("layers", c_int32), ("tile_w", c_int32), ("tile_h", c_int32),
                ("cblk_w_log2", c_int32), ("cblk_h_log2", c_int32), ("nprecincts", c_int32),
                ("prec_w_log2", c_int32 * 16), ("prec_h_log2", c_int32 * 16),
                ("progression", c_int32), ("sop", c_int32), ("eph", c_int32), ("plt", c_int32),
                ("tparts_r", c_int32), ("guard_bits", c_int32), ("reversible", c_int32),
                ("mct", c_int32), ("qstep", c_double), ("rate_bpp", c_double),
                ("format", c_int32), ("comment", c_int32), ("slope_skip", c_int32),
                ("flush_period", c_int32)]


class Organisation(Structure):
    """jp2hip_organisation: code-stream organisation that is no part of the
    recipe (Kakadu's ORG cluster).  All zero = none."""
    _fields_ = [("tlm", c_int32), ("reserved", c_int32 * 3)]


class Layout(Structure):
    _fields_ = [("width", c_int32), ("height", c_int32), ("components", c_int32),
                ("bits", c_int32), ("planar", c_int32), ("big_endian", c_int32),
                ("rows_per_strip", c_int32), ("nstrips", c_int32),
                ("strip_offsets", POINTER(c_uint64)),
                ("compression", c_int32), ("predictor", c_int32),
                ("strip_bytes", POINTER(c_uint64)),
                ("tile_width", c_int32), ("tile_height", c_int32),
                # what the source states about its pixels (zero: nothing), carried
                # into the JP2 / JPX header
                ("extra_samples", c_int32), ("res_unit", c_int32),
                ("xres_num", c_uint32), ("xres_den", c_uint32),
                ("yres_num", c_uint32), ("yres_den", c_uint32),
                ("icc", POINTER(c_uint8)), ("icc_bytes", c_uint64),
                # the pixel format (zero: BlackIsZero grey / RGB samples as they
                # are): bits may be 1, 2, 4; palette indices come with a colormap
                ("photometric", c_int32), ("fill_order", c_int32),
                ("colormap", POINTER(c_uint8)), ("colormap_entries", c_uint64)]

    METADATA = ("extra_samples", "res_unit", "xres_num", "xres_den", "yres_num", "yres_den")
    PIXEL_FORMAT = ("photometric", "fill_order", "colormap", "colormap_entries")

    def icc_profile(self) -> bytes:
        """The ICC profile bytes the layout points at (b"" when it has none)."""
        return ctypes.string_at(self.icc, self.icc_bytes) if self.icc and self.icc_bytes else b""

    def set_icc_profile(self, profile: bytes) -> None:
        """Point the layout at a copy of `profile` that lives as long as it does."""
        self._icc_keep = (c_uint8 * max(1, len(profile))).from_buffer_copy(profile or b"\0")
        self.icc = ctypes.cast(self._icc_keep, POINTER(c_uint8)) if profile else None
        self.icc_bytes = len(profile)

    def copy_metadata(self, src: "Layout") -> None:
        """Take `src`'s metadata fields (a band's layout keeps the file's)."""
        for name in Layout.METADATA:
            setattr(self, name, getattr(src, name))
        self.set_icc_profile(src.icc_profile())

    def colormap_bytes(self) -> bytes:
        """The ColorMap data the layout points at: colormap_entries 16-bit
        values in the file's byte order (b"" when it has none)."""
        n = 2 * self.colormap_entries
        return ctypes.string_at(self.colormap, n) if self.colormap and n else b""

    def set_colormap(self, data: bytes) -> None:
        """Point the layout at a copy of `data` (raw ColorMap values, two
        bytes each in the byte order `big_endian` names) that lives as long
        as it does."""
        if len(data) % 2:
            raise ValueError("a colormap holds 16-bit entries")
        self._colormap_keep = (c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
        self.colormap = ctypes.cast(self._colormap_keep, POINTER(c_uint8)) if data else None
        self.colormap_entries = len(data) // 2

    def copy_pixel_format(self, src: "Layout") -> None:
        """Take `src`'s pixel-format fields, the colormap as a copy."""
        self.photometric, self.fill_order = src.photometric, src.fill_order
        self.set_colormap(src.colormap_bytes())


class Stats(Structure):
    _fields_ = [("total_ms", c_double), ("h2d_ms", c_double), ("ingest_ms", c_double),
                ("dwt_ms", c_double), ("quant_ms", c_double), ("t1_ms", c_double),
                ("pcrd_ms", c_double), ("d2h_ms", c_double), ("t2_ms", c_double),
                ("codeblocks", c_int64), ("coded_passes", c_int64), ("t1_bytes", c_int64),
                ("out_bytes", c_int64), ("rate_iterations", c_int32), ("host_waits", c_int32),
                ("t1_cm_ms", c_double), ("t1_mq_ms", c_double), ("mq_decisions", c_int64),
                ("stream_pool_bytes", c_int64), ("stream_need_bytes", c_int64), ("pool_grows", c_int32),
                ("reused", c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LayerReport(Structure):
    """struct jp2hip_layer_report: per layer the threshold it was cut at,
    the code-stream bytes through it and (when enabled, else NaN) the
    predicted squared error left after it, summed over the image."""
    _fields_ = [("layers", c_int32), ("distortion_valid", c_int32), ("threshold", c_double * 32),
                ("bytes", c_int64 * 32), ("distortion", c_double * 32)]

    def psnr(self, l: int, width: int, height: int, components: int, bits: int) -> float:
        """The PSNR (dB) layer ``l``'s predicted distortion amounts to on a
        width x height image of ``components`` ``bits``-bit samples."""
        mse = self.distortion[l] / (width * height * components)
        peak = float((1 << bits) - 1)
        return math.inf if mse <= 0.0 else 10.0 * math.log10(peak * peak / mse)


# every symbol include/jp2hip.h declares
EXPORTS = ("jp2hip_version", "jp2hip_last_error", "jp2hip_probe", "jp2hip_device_count", "jp2hip_device_ordinals",
           "jp2hip_recipe_init",
           "jp2hip_create", "jp2hip_destroy", "jp2hip_encode_file", "jp2hip_encode_tiff",
           "jp2hip_tiff_layout", "jp2hip_encoded_format", "jp2hip_file_header", "jp2hip_encode_device", "jp2hip_free",
           # batch path (csrc/batch.cpp; bound in jp2hip.batch)
           "jp2hip_batch_create", "jp2hip_batch_submit", "jp2hip_batch_wait", "jp2hip_batch_pending",
           "jp2hip_batch_destroy",
           # tile-split path (csrc/split.cpp, encode.cpp, split_host.cpp; bound in jp2hip.split)
           "jp2hip_split_rows", "jp2hip_encode_device_split", "jp2hip_split_thresholds",
           "jp2hip_split_peers", "jp2hip_tiff_pixels", "jp2hip_env_check",
           # the progression order's packet sequence (api.cpp; host only)
           "jp2hip_packet_sequence",
           # code-stream organisation: TLM marker segments (api.cpp, batch.cpp; jp2hip_tlm_segments host only)
           "jp2hip_set_organisation", "jp2hip_batch_set_organisation", "jp2hip_tlm_segments",
           # tile-part divisions L and C (api.cpp, batch.cpp; jp2hip_tile_parts host only)
           "jp2hip_set_tile_part_divisions", "jp2hip_batch_set_tile_part_divisions", "jp2hip_tile_parts",
           # fixed-slope layers and the per-layer report (api.cpp, batch.cpp; the check host only)
           "jp2hip_set_layer_slopes", "jp2hip_batch_set_layer_slopes", "jp2hip_check_layer_slopes",
           "jp2hip_set_layer_report", "jp2hip_layer_report",
           # explicit per-layer rates (api.cpp, batch.cpp; the check, the step and the targets host only)
           "jp2hip_set_layer_rates", "jp2hip_batch_set_layer_rates", "jp2hip_check_layer_rates",
           "jp2hip_layer_rate_step", "jp2hip_layer_rate_targets",
           # quality layers by target PSNR (api.cpp, batch.cpp, split.cpp; all but the two setters host only)
           "jp2hip_set_layer_psnr", "jp2hip_batch_set_layer_psnr", "jp2hip_check_layer_psnr",
           "jp2hip_distortion_quantum", "jp2hip_layer_psnr_targets", "jp2hip_split_psnr_thresholds",
           "jp2hip_layer_psnr_fits",
           # source orientation, TIFF tag 274 (api.cpp, batch.cpp; the tag reader, the size and the rows host only)
           "jp2hip_set_source_orientation", "jp2hip_batch_set_source_orientation", "jp2hip_tiff_orientation",
           "jp2hip_oriented_size", "jp2hip_orientation_source_rows",
           # device-memory policy (api.cpp; csrc/context.h EncodeEnd)
           "jp2hip_device_bytes", "jp2hip_set_memory_limits", "jp2hip_device_memory", "jp2hip_dma_engines")
# ... but for the two whose names hold a digit, which the header scan of tests/test_abi.py does not read
# (host only; bound in lib() like the rest, tests/test_slopes.py calls them)
EXPORTS_WITH_DIGITS = ("jp2hip_slope_from_log2", "jp2hip_slope_to_log2")


# int (*)(void *user, int64_t *values, int32_t n): in-place sum over ranks, 0 ok
ALLREDUCE_FN = CFUNCTYPE(c_int, c_void_p, POINTER(c_int64), c_int32)


class Split(Structure):
    _fields_ = [("rank", c_int32), ("world", c_int32), ("allreduce_sum", ALLREDUCE_FN),
                ("user", c_void_p)]

_lib = None


def lib():
    """Load libjp2hip.so once; raise if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Jp2hipError(f"libjp2hip is not built ({LIB_PATH} missing); run __graft_entry__.build()")
    L = ctypes.CDLL(LIB_PATH)
    L.jp2hip_version.restype = c_char_p
    L.jp2hip_last_error.restype = c_char_p
    L.jp2hip_probe.restype = c_int
    L.jp2hip_device_count.restype = c_int
    L.jp2hip_device_ordinals.argtypes = [POINTER(c_int32), c_int32]
    L.jp2hip_device_ordinals.restype = c_int
    L.jp2hip_recipe_init.argtypes = [POINTER(Recipe), c_int]
    L.jp2hip_create.argtypes = [POINTER(c_void_p), POINTER(Config)]
    L.jp2hip_destroy.argtypes = [c_void_p]
    L.jp2hip_encode_file.argtypes = [c_void_p, c_char_p, c_char_p, c_int, POINTER(Recipe),
                                     POINTER(Stats)]
    L.jp2hip_encode_tiff.argtypes = [c_void_p, c_void_p, c_size_t, c_int, POINTER(Recipe),
                                     POINTER(POINTER(c_uint8)), POINTER(c_size_t), POINTER(Stats)]
    L.jp2hip_tiff_layout.argtypes = [c_void_p, c_size_t, POINTER(Layout), POINTER(c_uint64),
                                     c_int32]
    L.jp2hip_encoded_format.argtypes = [POINTER(Layout), POINTER(c_int32), POINTER(c_int32)]
    L.jp2hip_file_header.argtypes = [POINTER(Layout), c_int32, c_uint64, c_void_p, c_size_t]
    L.jp2hip_file_header.restype = c_int64
    L.jp2hip_encode_device.argtypes = [c_void_p, c_void_p, c_size_t, POINTER(Layout), c_int,
                                       POINTER(Recipe), POINTER(POINTER(c_uint8)),
                                       POINTER(c_size_t), POINTER(Stats)]
    L.jp2hip_free.argtypes = [c_void_p]
    L.jp2hip_split_rows.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32),
                                    POINTER(c_int32)]
    L.jp2hip_split_rows.restype = None
    L.jp2hip_encode_device_split.argtypes = [c_void_p, c_void_p, c_size_t, POINTER(Layout), c_int,
                                             POINTER(Recipe), POINTER(Split),
                                             POINTER(POINTER(c_uint8)), POINTER(c_size_t),
                                             POINTER(c_uint64), POINTER(c_uint64), POINTER(Stats)]
    L.jp2hip_split_peers.argtypes = [c_void_p, POINTER(c_int32), c_int32, c_int64]
    L.jp2hip_env_check.restype = c_char_p
    L.jp2hip_tiff_pixels.argtypes = [c_char_p]
    L.jp2hip_tiff_pixels.restype = c_int64
    L.jp2hip_split_thresholds.argtypes = [POINTER(c_uint64), POINTER(c_int64), c_int64,
                                          POINTER(c_int64), c_int32, POINTER(Split),
                                          POINTER(c_uint64)]
    L.jp2hip_packet_sequence.argtypes = [c_int32, c_int32, c_int32, c_int32, POINTER(Recipe), c_int32,
                                         POINTER(c_uint32), c_int64]
    L.jp2hip_packet_sequence.restype = c_int64
    L.jp2hip_set_organisation.argtypes = [c_void_p, POINTER(Organisation)]
    L.jp2hip_batch_set_organisation.argtypes = [c_void_p, POINTER(Organisation)]
    L.jp2hip_tlm_segments.argtypes = [POINTER(ctypes.c_uint16), POINTER(c_uint32), c_int64, c_void_p, c_size_t]
    L.jp2hip_tlm_segments.restype = c_int64
    L.jp2hip_set_tile_part_divisions.argtypes = [c_void_p, c_int32]
    L.jp2hip_batch_set_tile_part_divisions.argtypes = [c_void_p, c_int32]
    L.jp2hip_tile_parts.argtypes = [c_int32, c_int32, c_int32, c_int32, POINTER(Recipe), c_int32, c_int32,
                                    POINTER(c_uint32), c_int64]
    L.jp2hip_tile_parts.restype = c_int64
    L.jp2hip_set_layer_slopes.argtypes = [c_void_p, POINTER(c_double), c_int32]
    L.jp2hip_batch_set_layer_slopes.argtypes = [c_void_p, POINTER(c_double), c_int32]
    L.jp2hip_check_layer_slopes.argtypes = [POINTER(c_double), c_int32, POINTER(Recipe)]
    L.jp2hip_set_layer_rates.argtypes = [c_void_p, POINTER(c_double), c_int32]
    L.jp2hip_batch_set_layer_rates.argtypes = [c_void_p, POINTER(c_double), c_int32]
    L.jp2hip_check_layer_rates.argtypes = [POINTER(c_double), c_int32, POINTER(Recipe)]
    L.jp2hip_layer_rate_step.argtypes = [c_int32, c_int32, c_int64, c_int64, POINTER(c_int64), POINTER(c_int64),
                                         POINTER(c_int64)]
    L.jp2hip_layer_rate_targets.argtypes = [c_int32, c_int32, c_int32, c_int32, POINTER(Recipe), c_int32, c_int32,
                                            POINTER(c_double), c_int32, POINTER(c_int64), POINTER(c_int64),
                                            POINTER(c_int64)]
    L.jp2hip_set_layer_psnr.argtypes = [c_void_p, POINTER(c_double), c_int32]
    L.jp2hip_batch_set_layer_psnr.argtypes = [c_void_p, POINTER(c_double), c_int32]
    L.jp2hip_check_layer_psnr.argtypes = [POINTER(c_double), c_int32, POINTER(Recipe)]
    L.jp2hip_distortion_quantum.argtypes = [c_double, c_int64, c_int32]
    L.jp2hip_distortion_quantum.restype = c_int64
    L.jp2hip_layer_psnr_targets.argtypes = [c_int32, c_int32, c_int32, c_int32, POINTER(c_double), c_int32,
                                            POINTER(c_int64)]
    L.jp2hip_layer_psnr_fits.argtypes = [c_int32, c_int32, c_int32, c_int32, POINTER(Recipe)]
    L.jp2hip_split_psnr_thresholds.argtypes = [POINTER(c_uint64), POINTER(c_int64), c_int64,
                                               POINTER(c_int64), c_int32, POINTER(Split),
                                               POINTER(c_uint64)]
    L.jp2hip_slope_from_log2.argtypes = [c_double, c_int32]
    L.jp2hip_slope_from_log2.restype = c_double
    L.jp2hip_slope_to_log2.argtypes = [c_double, c_int32]
    L.jp2hip_slope_to_log2.restype = c_double
    L.jp2hip_set_layer_report.argtypes = [c_void_p, c_int32]
    L.jp2hip_layer_report.argtypes = [c_void_p, POINTER(LayerReport)]
    L.jp2hip_set_source_orientation.argtypes = [c_void_p, c_int32]
    L.jp2hip_batch_set_source_orientation.argtypes = [c_void_p, c_int32]
    L.jp2hip_tiff_orientation.argtypes = [c_void_p, c_size_t]
    L.jp2hip_tiff_orientation.restype = c_int32
    L.jp2hip_oriented_size.argtypes = [c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32)]
    L.jp2hip_orientation_source_rows.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32),
                                                 POINTER(c_int32)]
    L.jp2hip_device_bytes.argtypes = [c_void_p]
    L.jp2hip_device_bytes.restype = c_int64
    L.jp2hip_set_memory_limits.argtypes = [c_void_p, c_int64, c_int64]
    L.jp2hip_device_memory.argtypes = [c_int, POINTER(c_int64), POINTER(c_int64)]
    L.jp2hip_dma_engines.restype = c_char_p
    _lib = L
    return L


def last_error() -> str:
    return lib().jp2hip_last_error().decode("utf-8", "replace")


def version() -> str:
    return lib().jp2hip_version().decode()


def probe() -> bool:
    return bool(lib().jp2hip_probe())


def device_count() -> int:
    """gfx950 devices visible to libjp2hip (0 without a GPU)."""
    return int(lib().jp2hip_device_count())


def device_ordinals() -> list[int]:
    """HIP ordinals of the visible gfx950 devices (Encoder(device=...) takes these)."""
    n = int(lib().jp2hip_device_ordinals(None, 0))
    if n <= 0:
        return []
    buf = (c_int32 * n)()
    n = min(n, int(lib().jp2hip_device_ordinals(buf, n)))
    return [int(buf[i]) for i in range(n)]


def env_check() -> str:
    """"" or what the process environment should change for the contexts
    alive in it (jp2hip_env_check: GPU_MAX_HW_QUEUES)."""
    return lib().jp2hip_env_check().decode()


def dma_engines() -> str:
    """The SDMA engines the code-stream copies use and their probed rates."""
    return lib().jp2hip_dma_engines().decode()


def device_memory(device: int) -> tuple[int, int]:
    """(free, total) bytes of HIP device `device` (jp2hip_device_memory)."""
    fr, tot = c_int64(), c_int64()
    if lib().jp2hip_device_memory(device, byref(fr), byref(tot)) != 0:
        raise Jp2hipError(last_error())
    return int(fr.value), int(tot.value)


# what one context holds for the images a converter usually sees (C4-class
# 5000 x 7000 RGB8 lossless, DESIGN.md 3 "Footprint"); a pool is sized from it
CONTEXT_BUDGET_BYTES = 8 << 30


def contexts_for_memory(free_bytes: int, budget: int = CONTEXT_BUDGET_BYTES, cap: int = 16) -> int:
    """Contexts per GPU that fit 75 % of the device's free memory at `budget`
    bytes each (at least 1, at most `cap`)."""
    return max(1, min(cap, int(free_bytes * 0.75) // max(1, budget)))


def tiff_pixels(path) -> int:
    """Width x height of a TIFF file, from its header (jp2hip_tiff_pixels)."""
    n = int(lib().jp2hip_tiff_pixels(os.fsencode(path)))
    if n < 0:
        raise Jp2hipError(last_error())
    return n


def recipe(conversion: int, **overrides) -> Recipe:
    """The default recipe of `conversion` with `overrides` applied field by
    field (jp2hip.h, jp2hip_recipe).  ``tile_w=0, tile_h=0`` is the untiled
    recipe: one tile for the whole image, sized by the encode to the smallest
    multiples of 2^levels not below the image's width and height."""
    r = Recipe()
    lib().jp2hip_recipe_init(byref(r), conversion)
    for k, v in overrides.items():
        if k in ("prec_w_log2", "prec_h_log2"):
            arr = getattr(r, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(r, k, v)
    return r


def packet_sequence(width: int, height: int, components: int, bits: int, rcp: Recipe, tile: int) -> list[int]:
    """The packets of tile `tile` in the order ``rcp.progression`` sends them
    (jp2hip_packet_sequence; no GPU): entry s is ``p * layers + l`` for layer
    l of the tile's p-th precinct in (resolution, row, column, component)
    order -- RPCL gives 0, 1, 2, ...  Raises for a recipe the encodes refuse."""
    n = int(lib().jp2hip_packet_sequence(width, height, components, bits, byref(rcp), tile, None, 0))
    if n < 0:
        raise Jp2hipError(last_error())
    buf = (c_uint32 * max(1, n))()
    if int(lib().jp2hip_packet_sequence(width, height, components, bits, byref(rcp), tile, buf, n)) != n:
        raise Jp2hipError(last_error())
    return list(buf[:n])


TPARTS_L, TPARTS_C = 2, 4  # JP2HIP_TPARTS_L, JP2HIP_TPARTS_C


def tparts_letters(letters) -> int:
    """"L", "C", "LC" (any case and order; "" = none) or the bits themselves
    as the int jp2hip_set_tile_part_divisions takes.  "R" maps to bit 1, which
    the library refuses with a pointer at ``Recipe.tparts_r``."""
    if isinstance(letters, str):
        bits = {"R": 1, "L": TPARTS_L, "C": TPARTS_C}
        unknown = [ch for ch in letters.upper() if ch not in bits]
        if unknown:
            raise ValueError(f"tile-part divisions: {letters!r} has letters other than L and C")
        return sum({bits[ch] for ch in letters.upper()})
    return int(letters)


def tile_parts(width: int, height: int, components: int, bits: int, rcp: Recipe, letters, tile: int) -> list[int]:
    """The tile-parts of tile `tile` under ``rcp`` and the divisions `letters`
    (jp2hip_tile_parts; no GPU): the place in the tile's packet_sequence at
    which each starts, so their count is the list's length.  Raises for
    anything the encodes refuse (more than 255 tile-parts in a tile too)."""
    bits_ = tparts_letters(letters)
    n = int(lib().jp2hip_tile_parts(width, height, components, bits, byref(rcp), bits_, tile, None, 0))
    if n < 0:
        raise Jp2hipError(last_error())
    buf = (c_uint32 * max(1, n))()
    if int(lib().jp2hip_tile_parts(width, height, components, bits, byref(rcp), bits_, tile, buf, n)) != n:
        raise Jp2hipError(last_error())
    return list(buf[:n])


def slopes_array(slopes):
    """(ctypes double array or None, n) of a sequence of layer thresholds."""
    s = [float(x) for x in slopes] if slopes is not None else []
    return ((c_double * len(s))(*s) if s else None), len(s)


def check_layer_slopes(slopes, rcp: Recipe | None = None) -> None:
    """jp2hip_check_layer_slopes (no GPU): raises Jp2hipError, naming the
    entry, for thresholds jp2hip_set_layer_slopes -- or, with ``rcp``, an
    encode of that recipe -- refuses."""
    arr, n = slopes_array(slopes)
    if lib().jp2hip_check_layer_slopes(arr, n, byref(rcp) if rcp is not None else None) != 0:
        raise Jp2hipError(last_error())


def check_layer_psnr(psnr_db, rcp: Recipe | None = None) -> None:
    """jp2hip_check_layer_psnr (no GPU): raises Jp2hipError, naming the entry,
    for targets jp2hip_set_layer_psnr -- or, with ``rcp``, an encode of that
    recipe -- refuses."""
    arr, n = slopes_array(psnr_db)
    if lib().jp2hip_check_layer_psnr(arr, n, byref(rcp) if rcp is not None else None) != 0:
        raise Jp2hipError(last_error())


def distortion_quantum(weight: float, dd: int, bits: int) -> int:
    """jp2hip_distortion_quantum (no GPU): the integer one hull segment of
    distortion decrease ``dd`` in a block of PCRD weight ``weight`` adds to a
    selection by PSNR targets, for ``bits``-bit samples."""
    q = int(lib().jp2hip_distortion_quantum(weight, dd, bits))
    if q < 0:  # (quanta are never negative: the library's refusal of `bits`)
        raise Jp2hipError(last_error())
    return q


def layer_psnr_fits(width: int, height: int, components: int, bits: int, rcp: Recipe) -> bool:
    """jp2hip_layer_psnr_fits (no GPU): whether an encode of this image and
    recipe by PSNR targets is accepted -- False when its distortion quanta
    could overflow 63 bits.  Raises for a geometry or recipe no encode takes."""
    r = lib().jp2hip_layer_psnr_fits(width, height, components, bits, byref(rcp))
    if r < 0:
        raise Jp2hipError(last_error())
    return bool(r)


def layer_psnr_targets(width: int, height: int, components: int, bits: int, psnr_db) -> list[int]:
    """jp2hip_layer_psnr_targets (no GPU): the quanta each layer may leave in
    an image of this size for ``psnr_db`` (layer 0 first); -1 for a last 0, the
    lossless top layer."""
    arr, n = slopes_array(psnr_db)
    t = (c_int64 * 32)()
    if lib().jp2hip_layer_psnr_targets(width, height, components, bits, arr, n, t) != 0:
        raise Jp2hipError(last_error())
    return [int(x) for x in t[:n]]


def check_layer_rates(rates, rcp: Recipe | None = None) -> None:
    """jp2hip_check_layer_rates (no GPU): raises Jp2hipError, naming the
    entry, for rates jp2hip_set_layer_rates -- or, with ``rcp``, an encode of
    that recipe -- refuses."""
    arr, n = slopes_array(rates)
    if lib().jp2hip_check_layer_rates(arr, n, byref(rcp) if rcp is not None else None) != 0:
        raise Jp2hipError(last_error())


RATE_NO_BUDGET = (1 << 63) - 1  # the budget of a lossless top layer (no target: -1)


def layer_rate_step(it: int, fixed: int, part_bytes: int, layer_bytes, targets, budgets):
    """jp2hip_layer_rate_step (no GPU): one step of the per-layer rate loop
    after iteration ``it`` sized the code-stream.  Returns (halt, budgets):
    the budgets as the step leaves them (untouched when it halts)."""
    n = len(layer_bytes)
    if len(targets) != n or len(budgets) != n:
        raise ValueError("layer_bytes, targets and budgets differ in length")
    lb = (c_int64 * max(1, n))(*layer_bytes)
    t = (c_int64 * max(1, n))(*targets)
    b = (c_int64 * max(1, n))(*budgets)
    rc = int(lib().jp2hip_layer_rate_step(n, it, fixed, part_bytes, lb, t, b))
    if rc < 0:
        raise Jp2hipError(last_error())
    return bool(rc), list(b[:n])


def layer_rate_targets(width: int, height: int, components: int, bits: int, rcp: Recipe, rates, letters=0,
                       tlm: bool | int = 0):
    """jp2hip_layer_rate_targets (no GPU): (targets, first budgets, info) of an
    encode of this image by ``rates`` (layer 0 first); info = {"T", "E",
    "ntileparts", "npackets"}.  Raises for what the encodes refuse."""
    arr, n = slopes_array(rates)
    t = (c_int64 * 32)()
    b = (c_int64 * 32)()
    info = (c_int64 * 4)()
    if lib().jp2hip_layer_rate_targets(width, height, components, bits, byref(rcp), tparts_letters(letters),
                                       int(tlm), arr, n, t, b, info) != 0:
        raise Jp2hipError(last_error())
    return list(t[:n]), list(b[:n]), dict(zip(("T", "E", "ntileparts", "npackets"), (int(x) for x in info)))


def slope_from_log2(v: float, bits: int) -> float:
    """The threshold Kdu-Layer-Info prints as ``v`` for ``bits``-bit samples: 2^(v + 2 bits)."""
    return float(lib().jp2hip_slope_from_log2(v, bits))


def slope_to_log2(s: float, bits: int) -> float:
    """What Kdu-Layer-Info prints (before rounding) for threshold ``s``."""
    return float(lib().jp2hip_slope_to_log2(s, bits))


def tlm_segments(tiles, lengths) -> bytes:
    """The TLM marker segments (jp2hip_tlm_segments; no GPU) for tile-parts
    in file order: ``tiles[i]`` the tile index and ``lengths[i]`` the length
    (Psot) of the i-th.  Raises for more tile-parts than 256 segments hold."""
    n = len(tiles)
    if len(lengths) != n:
        raise ValueError("tiles and lengths differ in length")
    t = (ctypes.c_uint16 * max(1, n))(*tiles)
    ln = (c_uint32 * max(1, n))(*lengths)
    need = int(lib().jp2hip_tlm_segments(t, ln, n, None, 0))
    if need < 0:
        raise Jp2hipError(last_error())
    out = ctypes.create_string_buffer(max(1, need))
    if int(lib().jp2hip_tlm_segments(t, ln, n, out, need)) != need:
        raise Jp2hipError(last_error())
    return out.raw[:need]


def tiff_orientation(data: bytes) -> int:
    """TIFF tag 274 (Orientation) of a file (jp2hip_tiff_orientation; no GPU):
    its value when it is one SHORT in 1..8, 1 when it is absent or malformed.
    Raises when ``data`` is no TIFF at all."""
    o = int(lib().jp2hip_tiff_orientation(ctypes.create_string_buffer(data, len(data)), len(data)))
    if o < 0:
        raise Jp2hipError(last_error())
    return o


def oriented_size(width: int, height: int, o: int) -> tuple[int, int]:
    """(width, height) of the upright image of a stored width x height one
    under orientation ``o`` (jp2hip_oriented_size; no GPU)."""
    ow, oh = c_int32(), c_int32()
    if lib().jp2hip_oriented_size(width, height, o, byref(ow), byref(oh)) != 0:
        raise Jp2hipError(last_error())
    return ow.value, oh.value


def orientation_source_rows(height: int, width: int, o: int, row0: int, row1: int) -> tuple[int, int]:
    """The stored rows [s0, s1) that rows [row0, row1) of the upright image
    are made from (jp2hip_orientation_source_rows; no GPU): what a tile-split
    rank passes to ``split.band_strips`` for its band of upright rows."""
    s0, s1 = c_int32(), c_int32()
    if lib().jp2hip_orientation_source_rows(height, width, o, row0, row1, byref(s0), byref(s1)) != 0:
        raise Jp2hipError(last_error())
    return s0.value, s1.value


def tiff_layout(data: bytes):
    """Parse a baseline TIFF header; returns (Layout, offsets array).  The
    Layout owns copies of the file's ICC profile and ColorMap (Layout.icc and
    Layout.colormap point at them)."""
    lay = Layout()
    cap = 1 << 20
    offs = (c_uint64 * cap)()
    buf = ctypes.create_string_buffer(data, len(data))
    if lib().jp2hip_tiff_layout(buf, len(data), byref(lay), offs, cap) != 0:
        raise Jp2hipError(last_error())
    n = lay.nstrips
    packed = lay.compression > 1 or lay.tile_width > 0
    m = 2 * n if packed else n  # compressed / tiled: offsets, then byte counts
    keep = (c_uint64 * m)(*offs[:m])
    lay.strip_offsets = ctypes.cast(keep, POINTER(c_uint64))
    if packed:
        lay.strip_bytes = ctypes.cast(ctypes.byref(keep, 8 * n), POINTER(c_uint64))
    # the library pointed lay.icc and lay.colormap into `buf`, a temporary:
    # re-point them at copies the Layout keeps
    lay.set_icc_profile(lay.icc_profile())
    lay.set_colormap(lay.colormap_bytes())
    return lay, keep


def encoded_format(layout: Layout) -> tuple[int, int]:
    """(components, bits) of the code-stream this source is encoded as
    (jp2hip_encoded_format): 3 x 8 for a palette, 1 x 8 for 1-, 2- and 4-bit
    grey, else the layout's own."""
    nc, bits = c_int32(), c_int32()
    if lib().jp2hip_encoded_format(byref(layout), byref(nc), byref(bits)) != 0:
        raise Jp2hipError(last_error())
    return int(nc.value), int(bits.value)


def file_header(layout: Layout, fmt: int, codestream_bytes: int) -> bytes:
    """The bytes in front of the code-stream (signature .. jp2c box header)
    for this source description (jp2hip_file_header; no GPU): b"" for
    FORMAT_J2K."""
    n = int(lib().jp2hip_file_header(byref(layout), fmt, codestream_bytes, None, 0))
    if n < 0:
        raise Jp2hipError(last_error())
    out = ctypes.create_string_buffer(max(1, n))
    if int(lib().jp2hip_file_header(byref(layout), fmt, codestream_bytes, out, n)) != n:
        raise Jp2hipError(last_error())
    return out.raw[:n]


class _PinnedBuffer:
    """Owns one *out buffer of the encode calls; returns it to jp2hip's pool
    (jp2hip_free) when the last holder -- the Output or a view of it -- goes."""

    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            lib().jp2hip_free(self.ptr)
        except Exception:
            pass


class Output:
    """An encode's file bytes, left where the library wrote them (pinned host
    memory from jp2hip's pool) instead of copied into a Python bytes object.
    close() (or collection) releases the Output's hold; the buffer goes back
    to the pool once no view() of it is alive either, so a view never sees
    another encode's bytes."""

    def __init__(self, ptr, n: int):
        self._buf = _PinnedBuffer(ptr)
        self._n = n

    def __len__(self):
        return self._n

    def view(self) -> memoryview:
        if self._buf is None:
            raise ValueError("released output")
        arr = (c_uint8 * self._n).from_address(ctypes.addressof(self._buf.ptr.contents))
        arr._jp2hip_owner = self._buf  # the view keeps the pinned buffer alive
        return memoryview(arr)

    def tobytes(self) -> bytes:
        return bytes(self.view())

    def tail(self, k: int) -> bytes:
        """The last k bytes, read in place (no array type, no view)."""
        if self._buf is None:
            raise ValueError("released output")
        k = min(k, self._n)
        return ctypes.string_at(ctypes.addressof(self._buf.ptr.contents) + self._n - k, k)

    def close(self):
        self._buf = None


class Encoder:
    """One libjp2hip context bound to one GPU (thread-safe, calls serialise).
    The encode_* methods return the file as bytes, or with copy=False as an
    Output over the library's buffer (no host copy of the result)."""

    def __init__(self, device: int = 0, host_threads: int = 0, profile: bool = False):
        cfg = Config(device, host_threads, 1 if profile else 0, 0)
        h = c_void_p()
        if lib().jp2hip_create(byref(h), byref(cfg)) != 0:
            raise Jp2hipError(last_error())
        self._h = h

    def close(self):
        if self._h:
            lib().jp2hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_bytes(self) -> int:
        """Device memory held by this context (jp2hip_device_bytes)."""
        return int(lib().jp2hip_device_bytes(self._h))

    def set_memory_limits(self, soft: int = 0, hard: int = 0):
        """jp2hip_set_memory_limits: <= 0 keeps the default of each."""
        if lib().jp2hip_set_memory_limits(self._h, int(soft), int(hard)) != 0:
            raise Jp2hipError(last_error())

    def set_organisation(self, tlm: bool | int = 0, reserved=(0, 0, 0)):
        """jp2hip_set_organisation, for every later encode on this context and
        its tile-split peers: ``tlm`` = TLM marker segments in the main header
        (ORGgen_tlm).  Not while the context is encoding."""
        org = Organisation(int(tlm), (c_int32 * 3)(*reserved))
        if lib().jp2hip_set_organisation(self._h, byref(org)) != 0:
            raise Jp2hipError(last_error())

    def set_tile_part_divisions(self, letters=0):
        """jp2hip_set_tile_part_divisions, for every later encode on this
        context and its tile-split peers: "L", "C", "LC" or the bits
        (TPARTS_L | TPARTS_C); 0 restores the output without them.  R stays
        ``Recipe.tparts_r``.  Not while the context is encoding."""
        if lib().jp2hip_set_tile_part_divisions(self._h, tparts_letters(letters)) != 0:
            raise Jp2hipError(last_error())

    def set_layer_slopes(self, slopes=None):
        """jp2hip_set_layer_slopes, for every later encode on this context and
        its tile-split peers: one threshold per layer, layer 0 first, none
        increasing (the last 0 for a lossless recipe); None or () turns the
        fixed slopes off.  Not while the context is encoding."""
        arr, n = slopes_array(slopes)
        if lib().jp2hip_set_layer_slopes(self._h, arr, n) != 0:
            raise Jp2hipError(last_error())

    def set_layer_psnr(self, psnr_db=None):
        """jp2hip_set_layer_psnr, for every later encode on this context and
        its tile-split peers: layer l is the smallest selection whose predicted
        PSNR is at least ``psnr_db[l]`` dB (OpenJPEG's ``-q``), layer 0 first
        and none decreasing.  With ``Recipe.rate_bpp <= 0`` the last entry
        must be 0: the top layer takes every coded pass.  There is no byte
        target and no rate loop; ``layer_report().threshold`` holds the slopes
        the layers were cut at.  None or () turns the targets off; targets,
        rates and fixed slopes exclude one another.  Not while the context is
        encoding."""
        arr, n = slopes_array(psnr_db)
        if lib().jp2hip_set_layer_psnr(self._h, arr, n) != 0:
            raise Jp2hipError(last_error())

    def set_layer_rates(self, rates=None):
        """jp2hip_set_layer_rates, for every later encode on this context and
        its tile-split peers: ``rates[l]`` (bits per pixel) bounds the
        code-stream through layer l, layer 0 first and none decreasing --
        Kakadu's ``-rate`` lists the highest rate first, so ``-rate 3,1.5,0.75``
        is ``[0.75, 1.5, 3]`` here.  For a lossless recipe the last entry is 0
        (``-rate -,1.5,0.75`` is ``[0.75, 1.5, 0]``): the top layer takes every
        coded pass.  ``Recipe.rate_bpp`` is then no target.  None or () turns
        the rates off; rates and fixed slopes exclude each other.  Not while
        the context is encoding."""
        arr, n = slopes_array(rates)
        if lib().jp2hip_set_layer_rates(self._h, arr, n) != 0:
            raise Jp2hipError(last_error())

    def set_source_orientation(self, o: int = ORIENT_OFF):
        """jp2hip_set_source_orientation, for every later encode on this
        context and its tile-split peers: ORIENT_OFF (the default: the rows as
        stored, whatever the tag says), a TIFF Orientation 1..8, or
        ORIENT_TIFF, the file's own tag 274 (encode_file, encode_tiff and the
        batch queue; encode_device takes a layout and is refused under it --
        read the tag with ``tiff_orientation`` and set its value).  The file
        holds the upright pixels.  Not while the context is encoding."""
        if lib().jp2hip_set_source_orientation(self._h, int(o)) != 0:
            raise Jp2hipError(last_error())

    def set_layer_report(self, on: bool | int = True):
        """jp2hip_set_layer_report: later encodes also sum the distortion
        every layer leaves (one small kernel pair and a host wait more)."""
        if lib().jp2hip_set_layer_report(self._h, int(on)) != 0:
            raise Jp2hipError(last_error())

    def layer_report(self) -> LayerReport:
        """jp2hip_layer_report: the last successful encode's layers."""
        r = LayerReport()
        if lib().jp2hip_layer_report(self._h, byref(r)) != 0:
            raise Jp2hipError(last_error())
        return r

    def _take(self, out, n, copy=True):
        if not copy:
            return Output(out, n.value)
        try:
            return ctypes.string_at(out, n.value)
        finally:
            lib().jp2hip_free(out)

    def encode_tiff(self, data: bytes, conversion: int, rcp: Recipe | None = None):
        out = POINTER(c_uint8)()
        n = c_size_t()
        st = Stats()
        buf = ctypes.create_string_buffer(data, len(data))
        rc = lib().jp2hip_encode_tiff(self._h, buf, len(data), conversion,
                                      byref(rcp) if rcp is not None else None,
                                      byref(out), byref(n), byref(st))
        if rc != 0:
            raise Jp2hipError(last_error())
        return self._take(out, n), st

    def encode_tiff_ptr(self, h_ptr: int, nbytes: int, conversion: int, rcp: Recipe | None = None,
                        copy: bool = True):
        """encode_tiff on TIFF bytes already in host memory at h_ptr (pinned
        memory makes the H2D a plain DMA)."""
        out = POINTER(c_uint8)()
        n = c_size_t()
        st = Stats()
        rc = lib().jp2hip_encode_tiff(self._h, c_void_p(h_ptr), nbytes, conversion,
                                      byref(rcp) if rcp is not None else None,
                                      byref(out), byref(n), byref(st))
        if rc != 0:
            raise Jp2hipError(last_error())
        return self._take(out, n, copy), st

    def encode_device(self, d_ptr: int, nbytes: int, layout: Layout, conversion: int,
                      rcp: Recipe | None = None, copy: bool = True):
        out = POINTER(c_uint8)()
        n = c_size_t()
        st = Stats()
        rc = lib().jp2hip_encode_device(self._h, c_void_p(d_ptr), nbytes, byref(layout), conversion,
                                        byref(rcp) if rcp is not None else None,
                                        byref(out), byref(n), byref(st))
        if rc != 0:
            raise Jp2hipError(last_error())
        return self._take(out, n, copy), st

    def encode_device_split(self, d_ptr: int, nbytes: int, layout: Layout, conversion: int,
                            split: Split, rcp: Recipe | None = None):
        """This rank's part of a tile-split encode: (bytes, file_offset, file_len, Stats)."""
        out = POINTER(c_uint8)()
        n = c_size_t()
        off = c_uint64()
        flen = c_uint64()
        st = Stats()
        rc = lib().jp2hip_encode_device_split(self._h, c_void_p(d_ptr), nbytes, byref(layout),
                                              conversion, byref(rcp) if rcp is not None else None,
                                              byref(split), byref(out), byref(n), byref(off),
                                              byref(flen), byref(st))
        if rc != 0:
            raise Jp2hipError(last_error())
        return self._take(out, n), off.value, flen.value, st

    def split_peers(self, ordinals: list[int], min_pixels: int = 0):
        """Tile-split this encoder's images of >= min_pixels pixels across
        itself and one peer context per entry of ``ordinals``
        (jp2hip_split_peers); ``[]`` removes the peers."""
        arr = (c_int32 * max(1, len(ordinals)))(*ordinals)
        if lib().jp2hip_split_peers(self._h, arr, len(ordinals), min_pixels) != 0:
            raise Jp2hipError(last_error())

    def encode_file(self, tiff_path: str, out_path: str, conversion: int,
                    rcp: Recipe | None = None):
        st = Stats()
        rc = lib().jp2hip_encode_file(self._h, os.fsencode(tiff_path), os.fsencode(out_path),
                                      conversion, byref(rcp) if rcp is not None else None,
                                      byref(st))
        if rc != 0:
            raise Jp2hipError(last_error())
        return st
