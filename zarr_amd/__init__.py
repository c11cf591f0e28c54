"""zarr_amd — MI355X-native Zarr chunk-codec path.

Drop-in for the chunk encode/decode path of sci-rs/zarr v0.0.1
(``src/chunk.rs`` + ``src/compression``): every ``CompressionType`` chunk is
decoded/encoded by hand-written gfx950 HIP kernels behind the C ABI in
``include/zchunk_gpu.h``.  The Python layer mirrors the reference's types so
callers (and the parity tests) read like the reference's own.
"""
from .compression import GZIP_CODEC_ID, Bzip2, CompressionType, Gzip, Lz4, Raw, Xz, Zlib
from .data_type import (DataType, Endian, ExtendedDataType, MetadataError, NATIVE_ENDIAN,
                        REFLECTED_TYPES, effective_type, zarr_type)
from .metadata import ArrayMetadata, u64_ceil_div
from .chunk import (DefaultChunk, SliceDataChunk, VecDataChunk, ZarrIOError, check_array_type,
                    read_chunks_host)
from .storage import FilesystemHierarchy, get_chunk_key
from .region import (BoundingBox, assemble_ortho, assemble_points, assemble_regions_s, points_grid, points_last, read_ndarray,
                     read_ndarrays, read_ndarrays_s, read_ndarrays_v, read_points,
                     region_s_chunks, regions_s_grid, regions_s_scratch_bytes, regions_s_waves, sboxes_tensor,
                     scatter_points, scatter_regions_s, write_ndarray, write_ndarrays, write_ndarrays_s,
                     write_ndarrays_v, write_points, ortho_chunks, ortho_scratch_bytes, read_ortho,
                     scatter_ortho, write_ortho)
from ._native import NativeUnavailable

__all__ = [
    "ArrayMetadata", "BoundingBox", "Bzip2", "CompressionType", "DataType", "DefaultChunk", "Endian",
    "ExtendedDataType", "FilesystemHierarchy", "GZIP_CODEC_ID", "Gzip", "Lz4", "MetadataError",
    "NATIVE_ENDIAN", "NativeUnavailable", "REFLECTED_TYPES", "Raw", "SliceDataChunk",
    "VecDataChunk", "Xz", "ZarrIOError", "Zlib", "check_array_type", "effective_type", "get_chunk_key",
    "assemble_regions_s", "read_chunks_host", "read_ndarray", "read_ndarrays", "read_ndarrays_s", "read_ndarrays_v",
    "region_s_chunks", "regions_s_grid", "regions_s_scratch_bytes", "regions_s_waves", "sboxes_tensor",
    "scatter_regions_s", "u64_ceil_div", "write_ndarray", "write_ndarrays", "write_ndarrays_s", "write_ndarrays_v",
    "zarr_type",
    "assemble_points", "points_grid", "points_last", "read_points", "scatter_points", "write_points",
    "assemble_ortho", "ortho_chunks", "ortho_scratch_bytes", "read_ortho", "scatter_ortho", "write_ortho",
]
