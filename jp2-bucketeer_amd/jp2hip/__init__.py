"""jp2hip -- MI355X JPEG 2000 encoder behind Bucketeer's converter API.

``jp2hip.converters`` mirrors src/main/java/edu/ucla/library/bucketeer/converters;
``jp2hip._lib`` binds the C ABI of libjp2hip (include/jp2hip.h).
"""
from ._lib import (FORMAT_J2K, FORMAT_JP2, FORMAT_JPX, LOSSLESS, LOSSY, ORDER_CPRL, ORDER_LRCP, ORDER_PCRL,
                   ORDER_RLCP, ORDER_RPCL, ORIENT_OFF, ORIENT_TIFF, Encoder, Jp2hipError, LayerReport, Output, check_layer_psnr, check_layer_rates, check_layer_slopes,
                   distortion_quantum, layer_psnr_fits, layer_psnr_targets,
                   device_count, device_ordinals, encoded_format, file_header, orientation_source_rows, oriented_size,
                   packet_sequence, probe, recipe, slope_from_log2, slope_to_log2, tiff_layout, tiff_orientation,
                   tile_parts, tlm_segments, version)
from .converters import (Conversion, Converter, ConverterFactory, GpuConverter,
                         KakaduConverter, KakaduNotFoundError, OpenJPEGConverter)

__all__ = ["Conversion", "Converter", "ConverterFactory", "GpuConverter", "KakaduConverter",
           "KakaduNotFoundError", "OpenJPEGConverter", "Encoder", "Jp2hipError", "LOSSY",
           "LOSSLESS", "FORMAT_J2K", "FORMAT_JP2", "FORMAT_JPX", "ORDER_LRCP", "ORDER_RLCP", "ORDER_RPCL",
           "ORDER_PCRL", "ORDER_CPRL", "LayerReport", "Output", "check_layer_psnr", "check_layer_rates", "check_layer_slopes",
           "distortion_quantum", "layer_psnr_fits", "layer_psnr_targets", "device_count",
           "device_ordinals", "encoded_format", "file_header", "packet_sequence", "probe", "recipe",
           "slope_from_log2", "slope_to_log2", "tiff_layout", "tile_parts", "tlm_segments", "version",
           "ORIENT_OFF", "ORIENT_TIFF", "orientation_source_rows", "oriented_size", "tiff_orientation"]
