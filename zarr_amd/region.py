"""Region assembly on the device — ``ZarrNdarrayReader`` (src/ndarray.rs).

``read_ndarray`` / ``read_ndarray_into`` (ndarray.rs:153-268) read every
chunk that ``bounded_coord_iter`` (ndarray.rs:410-432) visits from the
FilesystemHierarchy, decode them in one batch on the GPU (the chunk-codec hot
path), and scatter them into the bounding box with ``zcg_read_region`` — the
decoded chunks never leave HBM.  ``BoundingBox`` mirrors ndarray.rs:42-149.
"""
from __future__ import annotations

import ctypes
import itertools
import os
from typing import List, Sequence

import numpy as np

from . import _native
from .batch import BatchCodec
from .chunk import ZarrIOError, _raise_status, check_array_type
from .metadata import ArrayMetadata


class BoundingBox:
    """ndarray.rs:42-149 (offset/shape per dimension, u64)."""

    def __init__(self, offset: Sequence[int], shape: Sequence[int]):
        assert len(offset) == len(shape)
        self.offset = [int(o) for o in offset]
        self.shape = [int(s) for s in shape]

    def intersect(self, other: "BoundingBox") -> None:
        """ndarray.rs:71-85 (saturating)."""
        for d in range(len(self.offset)):
            new_o = max(other.offset[d], self.offset[d])
            self.shape[d] = max(0, min(self.shape[d] + self.offset[d], other.offset[d] + other.shape[d]) - new_o)
            self.offset[d] = new_o

    def union(self, other: "BoundingBox") -> None:
        """ndarray.rs:95-109."""
        for d in range(len(self.offset)):
            new_o = min(other.offset[d], self.offset[d])
            self.shape[d] = max(self.shape[d] + self.offset[d], other.offset[d] + other.shape[d]) - new_o
            self.offset[d] = new_o

    def end(self) -> List[int]:
        return [o + s for o, s in zip(self.offset, self.shape)]

    def is_empty(self) -> bool:
        return 0 in self.shape

    def __eq__(self, other) -> bool:
        return isinstance(other, BoundingBox) and self.offset == other.offset and self.shape == other.shape

    def __repr__(self) -> str:
        return f"BoundingBox(offset={self.offset}, shape={self.shape})"


def effective_fill_value(meta: ArrayMetadata, t) -> int:
    """lib.rs:448-454: the metadata fill_value as T, else T::default()."""
    v = meta.fill_value
    a = np.array(0 if v is None else v, dtype=np.dtype(t).newbyteorder("="))
    return int.from_bytes(a.tobytes().ljust(8, b"\0"), "little")


def _region(meta: ArrayMetadata, bbox: BoundingBox, es: int, fill: bool, fill_value: int,
            out_strides: Sequence[int]) -> _native.Region:
    nd = meta.get_ndim()
    if nd > _native.MAX_DIMS:
        raise _native.NativeUnavailable(f"region assembly supports up to {_native.MAX_DIMS} dimensions")
    r = _native.Region()
    r.ndim = nd
    r.elem_size = es
    r.chunk_order = 1 if meta.chunk_memory_layout == "F" else 0
    r.fill_missing = 1 if fill else 0
    for d in range(nd):
        r.array_shape[d] = meta.shape[d]
        r.chunk_shape[d] = meta.chunk_shape[d]
        r.bbox_offset[d] = bbox.offset[d]
        r.bbox_shape[d] = bbox.shape[d]
        r.out_strides[d] = int(out_strides[d])
    r.fill_value = fill_value
    return r


def region_grid(meta: ArrayMetadata, bbox: BoundingBox):
    """bounded_coord_iter's grid range (ndarray.rs:410-432) -> (lo, n)."""
    L = _native.load_library()
    nd = meta.get_ndim()
    r = _region(meta, bbox, 1, False, 0, [0] * nd)
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)()
    n = (ctypes.c_uint64 * _native.MAX_DIMS)()
    L.zcg_region_grid(ctypes.byref(r), ctypes.addressof(lo), ctypes.addressof(n))
    return [int(lo[d]) for d in range(nd)], [int(n[d]) for d in range(nd)]


def _strides(shape: Sequence[int], order: str) -> List[int]:
    st, acc = [0] * len(shape), 1
    dims = range(len(shape)) if order == "F" else reversed(range(len(shape)))
    for d in dims:
        st[d] = acc
        acc *= max(int(shape[d]), 1)
    return st


def _stream_handle(stream, device: int) -> int:
    """The native handle of `stream` (a torch stream or a raw handle); None:
    the device's current stream."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return s.cuda_stream if hasattr(s, "cuda_stream") else int(s)


def assemble_region(meta: ArrayMetadata, bbox: BoundingBox, es: int, table, out, out_strides,
                    fill: bool, fill_value: int, device: int = 0, stream=None) -> None:
    """Device-level call: `table` = device int64 tensor of chunk pointers
    (C order over region_grid's range, 0 = absent), `out` = device tensor
    whose data_ptr() is element (0, ..., 0) of the output view."""
    ctx = _native.context(device)
    r = _region(meta, bbox, es, fill, fill_value, out_strides)
    st = ctx.lib.zcg_read_region(ctx.handle, ctypes.byref(r), table.data_ptr() if table is not None else None,
                                 out.data_ptr(), _stream_handle(stream, device))
    _raise_status(st, ctx, "read_region")


def scatter_region(meta: ArrayMetadata, bbox: BoundingBox, es: int, table, box, box_strides, device: int = 0,
                   stream=None) -> None:
    """Device-level inverse of assemble_region (zcg_write_region): the box
    (`box` = device tensor whose data_ptr() is element (0, ..., 0) of a view
    with `box_strides`) is written into the chunk slots of `table`."""
    ctx = _native.context(device)
    r = _region(meta, bbox, es, False, 0, box_strides)
    st = ctx.lib.zcg_write_region(ctx.handle, ctypes.byref(r), table.data_ptr() if table is not None else None,
                                  box.data_ptr(), _stream_handle(stream, device))
    _raise_status(st, ctx, "write_region")


# write_ndarray works through the touched chunks in sub-batches of at most this
# many bytes of decoded slots plus encode capacity (device memory bound)
WRITE_BATCH_BYTES = 1 << 30


def _decode_visited(hier, path_name: str, meta: ArrayMetadata, bbox: BoundingBox, device: int, flags: int = 0):
    """Read + batch-decode the chunks bounded_coord_iter visits, through the
    store's get() semantics (shared flock, filesystem.rs:201-210) straight
    into device slots (zcg_store_read_chunks_device); returns (table tensor,
    keep-alive objects).  An absent chunk is skipped (ndarray.rs:229-231)."""
    import torch
    from .storage import store_read_device
    lo, n = region_grid(meta, bbox)
    coords = list(itertools.product(*[range(l, l + k) for l, k in zip(lo, n)]))  # C order
    for c in coords:
        assert meta.in_bounds(c)  # storage.rs:217 (read_chunk panics out of bounds)
    dev = torch.device("cuda", device)
    table = np.zeros(max(len(coords), 1), np.int64)
    keep = []
    if coords:
        es = meta.effective_type().size_of()
        D = meta.get_chunk_num_elements() * es
        slots = torch.empty(max(len(coords) * D, 1), dtype=torch.uint8, device=dev)
        ptrs = [slots.data_ptr() + i * D for i in range(len(coords))]
        st = store_read_device(meta, [hier.chunk_path(path_name, meta, c) for c in coords], ptrs, device,
                               flags=flags)
        for i, c in enumerate(coords):
            if st[i] == _native.ABSENT:
                continue  # read_chunk -> Ok(None)
            if st[i] != _native.OK:
                raise ZarrIOError(_native.STATUS_NAMES.get(int(st[i]), str(st[i])), f"chunk {list(c)}")
            table[i] = ptrs[i]
        keep.append(slots)
    return torch.from_numpy(table).to(dev), keep


def read_ndarray(hier, path_name: str, meta: ArrayMetadata, bbox: BoundingBox, t, device: int = 0,
                 as_tensor: bool = False, flags: int = 0):
    """ZarrNdarrayReader::read_ndarray (ndarray.rs:153-174): an array of the
    box's shape in the chunk memory order, fill value where no chunk is.
    `flags`: decode flags; under _native.FLAG_VERIFY* a chunk that fails its
    checksum raises InvalidData."""
    import torch
    check_array_type(t, meta)
    if len(bbox.offset) != meta.get_ndim():
        raise ZarrIOError("InvalidData", "Wrong number of dimensions")
    dt = np.dtype(t).newbyteorder("=")
    es = dt.itemsize
    order = "F" if meta.chunk_memory_layout == "F" else "C"
    st = _strides(bbox.shape, order)
    total = int(np.prod(bbox.shape)) if bbox.shape else 1
    out = torch.empty(max(total * es, 1), dtype=torch.uint8, device=torch.device("cuda", device))
    table, keep = _decode_visited(hier, path_name, meta, bbox, device, flags)
    assemble_region(meta, bbox, es, table, out, st, True, effective_fill_value(meta, dt), device)
    torch.cuda.synchronize(device)
    if as_tensor:
        return out[: total * es], st
    host = out[: total * es].cpu().numpy()
    return np.ndarray(tuple(bbox.shape), dtype=dt, buffer=host, strides=tuple(s * es for s in st)).copy(order=order)


def assemble_regions(meta: ArrayMetadata, shape: Sequence[int], es: int, table, table_lo, table_n, boxes, status,
                     out_strides, fill: bool, fill_value: int, device: int = 0, stream=None) -> None:
    """Device-level call for many boxes of one `shape` (zcg_read_regions):
    `table` = device int64 tensor of chunk pointers over the grid range
    table_lo .. table_lo + table_n (C order, 0 = absent), `boxes` = device
    tensor holding one _native.Box per box (offset per dim, output base),
    `status` = device int32 tensor, one word per box.  Asynchronous."""
    ctx = _native.context(device)
    nd = meta.get_ndim()
    r = _region(meta, BoundingBox([0] * nd, shape), es, fill, fill_value, out_strides)
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in table_lo])
    n = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in table_n])
    n_boxes = boxes.numel() * boxes.element_size() // ctypes.sizeof(_native.Box) if boxes is not None else 0
    st = ctx.lib.zcg_read_regions(ctx.handle, ctypes.byref(r), ctypes.addressof(lo), ctypes.addressof(n),
                                  table.data_ptr() if table is not None else None,
                                  boxes.data_ptr() if n_boxes else None, n_boxes,
                                  status.data_ptr() if status is not None else None,
                                  _stream_handle(stream, device))
    _raise_status(st, ctx, "read_regions")


def _native_meta(meta: ArrayMetadata, flags: int):
    st, am, msg = _native.array_meta_from_json(meta.to_json())
    if st != _native.OK:
        raise ZarrIOError(_native.STATUS_NAMES.get(st, str(st)), f"array metadata: {msg}")
    am.array.compression.flags = flags
    return am


class _StoreCall:
    """One store-level native call, prepared: the native metadata (`am`), the
    context, and the encoded root and path.  call(what, name, *args) runs
    lib.<name>(ctx, am, root, path, *args) and raises what a status other than
    OK stands for, with `what` before the context's message."""

    def __init__(self, hier, path_name: str, meta: ArrayMetadata, flags: int, device: int):
        self.am = _native_meta(meta, flags)
        self.ctx = _native.context(device)
        self.head = (self.ctx.handle, ctypes.byref(self.am), os.fsencode(hier.base_path), path_name.encode())

    def __call__(self, what: str, name: str, *args) -> None:
        r = getattr(self.ctx.lib, name)(*self.head, *args)
        if r != _native.OK:
            raise ZarrIOError(_native.STATUS_NAMES.get(r, str(r)), f"{what}: {self.ctx.last_error()}")


def _u64(rows, nd: int) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(rows, dtype=np.uint64).reshape(-1, nd))


class _Boxes:
    """A list of B boxes as the store-level calls take them: offsets, shapes
    and optional steps as contiguous B x ndim uint64 arrays (offs, shp, stp),
    every box's dense element strides in the chunk memory order, and the byte
    offsets `at` (B + 1) of the boxes back to back."""

    def __init__(self, meta: ArrayMetadata, offsets, shapes, es: int, steps=None):
        nd = meta.get_ndim()
        self.order = "F" if meta.chunk_memory_layout == "F" else "C"
        self.es = es
        self.shapes = [tuple(s) for s in shapes]
        self.B = len(self.shapes)
        self.offs, self.shp, self.stp = _u64(offsets, nd), _u64(self.shapes, nd), steps
        known, self.strides, self.at = {}, [], [0]
        for s in self.shapes:
            if s not in known:
                known[s] = _strides(s, self.order), int(np.prod(s, dtype=object)) * es
            self.strides.append(list(known[s][0]))  # a list of its own per box, as a caller may change it
            self.at.append(self.at[-1] + known[s][1])

    def pointers(self, base: int):
        """Box b's address when the boxes lie back to back from `base`."""
        return (ctypes.c_void_p * max(self.B, 1))(*[base + a for a in self.at[:-1]])

    def out(self, device=None):
        """Memory for the boxes back to back: host bytes, or with `device` a
        uint8 tensor -> (buffer, pointers)."""
        if device is None:
            buf = np.empty(max(self.at[-1], 1), np.uint8)
            return buf, self.pointers(buf.ctypes.data)
        import torch
        buf = torch.empty(max(self.at[-1], 1), dtype=torch.uint8, device=torch.device("cuda", device))
        return buf, self.pointers(buf.data_ptr())

    def views(self, host: np.ndarray, dt) -> list:
        """The boxes in `host` (out()'s bytes) as arrays, not copied."""
        return [np.ndarray(s, dtype=dt, buffer=host, offset=self.at[b],
                           strides=tuple(k * self.es for k in self.strides[b])) for b, s in enumerate(self.shapes)]


def _dense_inputs(meta: ArrayMetadata, arrays):
    """Host input boxes, each dense in the chunk memory order -> (the dense
    arrays, which own the memory; their shapes B x ndim; the pointer array)."""
    nd = meta.get_ndim()
    arrays = [np.asarray(a) for a in arrays]
    dense = []
    for a in arrays:
        if a.ndim != nd:
            raise ZarrIOError("InvalidData", "Wrong number of dimensions")
        dt = a.dtype.newbyteorder("=")
        check_array_type(dt, meta)
        dense.append(np.ascontiguousarray(a.astype(dt, copy=False).T if meta.chunk_memory_layout == "F"
                                          else a.astype(dt, copy=False)))
    ins = (ctypes.c_void_p * max(len(dense), 1))(*[a.ctypes.data if a.size else 0 for a in dense])
    return dense, _u64([a.shape for a in arrays], nd), ins


def read_ndarrays(hier, path_name: str, meta: ArrayMetadata, offsets, shape: Sequence[int], t, device: int = 0,
                  as_tensor: bool = False, flags: int = 0, slot_budget_bytes: int = 0):
    """read_ndarray for many boxes of one `shape` in one native call
    (zcg_store_read_boxes[_device]): an array of shape (B, *shape) whose [b]
    equals read_ndarray(..., BoundingBox(offsets[b], shape), t).  The chunks
    the boxes share are read and decoded once; `slot_budget_bytes` bounds the
    decoded chunks held on the device at a time (0: 4 GiB).  With as_tensor the
    result is (uint8 device tensor of B boxes back to back, element strides of
    one box), as read_ndarray gives for one."""
    check_array_type(t, meta)
    shape = [int(x) for x in shape]
    offs = _u64(offsets, len(shape))
    if len(shape) != meta.get_ndim():
        raise ZarrIOError("InvalidData", "Wrong number of dimensions")
    dt = np.dtype(t).newbyteorder("=")
    bx = _Boxes(meta, offs, [shape] * offs.shape[0], dt.itemsize)
    strides = _strides(shape, bx.order)
    call = _StoreCall(hier, path_name, meta, flags, device)
    bshape = (ctypes.c_uint64 * _native.MAX_DIMS)(*shape)
    buf, outs = bx.out(device if as_tensor else None)
    tail = (bx.offs.ctypes.data, ctypes.addressof(outs), bx.B, slot_budget_bytes, 16)
    if as_tensor:
        ostr = (ctypes.c_int64 * _native.MAX_DIMS)(*strides)
        call("read_boxes", "zcg_store_read_boxes_device", ctypes.addressof(bshape), ctypes.addressof(ostr), 1, *tail)
        return buf[: bx.at[-1]], strides
    call("read_boxes", "zcg_store_read_boxes", ctypes.addressof(bshape), *tail)
    res = np.empty((bx.B, *shape), dtype=dt, order="C")
    for b, box in enumerate(bx.views(buf, dt)):
        res[b] = box
    return res


def scatter_regions(meta: ArrayMetadata, shape: Sequence[int], es: int, table, table_lo, table_n, boxes, status,
                    box_strides, device: int = 0, stream=None) -> None:
    """Device-level inverse of assemble_regions (zcg_write_regions): every box
    (`boxes` = device tensor of _native.Box records whose `out` is element
    (0, ..., 0) of the box's input view with `box_strides`) is written into the
    chunk slots of `table`.  Boxes of one call that overlap leave either value;
    split the call with regions_waves where the later box must win.
    Asynchronous."""
    ctx = _native.context(device)
    nd = meta.get_ndim()
    r = _region(meta, BoundingBox([0] * nd, shape), es, False, 0, box_strides)
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in table_lo])
    n = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in table_n])
    n_boxes = boxes.numel() * boxes.element_size() // ctypes.sizeof(_native.Box) if boxes is not None else 0
    st = ctx.lib.zcg_write_regions(ctx.handle, ctypes.byref(r), ctypes.addressof(lo), ctypes.addressof(n),
                                   table.data_ptr() if table is not None else None,
                                   boxes.data_ptr() if n_boxes else None, n_boxes,
                                   status.data_ptr() if status is not None else None,
                                   _stream_handle(stream, device))
    _raise_status(st, ctx, "write_regions")


def _grid(name: str, meta: ArrayMetadata, bound, *rows):
    """A zcg_*_grid call (host code, no GPU) over `rows` (each B x ndim: the
    offsets, then what else the call takes per box) -> (lo, n)."""
    L = _native.load_library()
    nd = meta.get_ndim()
    r = _region(meta, BoundingBox([0] * nd, bound), 1, False, 0, [0] * nd)
    rows = [_u64(x, nd) for x in rows]
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)()
    n = (ctypes.c_uint64 * _native.MAX_DIMS)()
    getattr(L, name)(ctypes.byref(r), *[x.ctypes.data for x in rows], rows[0].shape[0], ctypes.addressof(lo),
                     ctypes.addressof(n))
    return [int(lo[d]) for d in range(nd)], [int(n[d]) for d in range(nd)]


def _waves(name: str, meta: ArrayMetadata, bound, *rows):
    """A zcg_*_waves call (host code, no GPU) over `rows` as for _grid ->
    (number of waves, wave index per box)."""
    L = _native.load_library()
    nd = meta.get_ndim()
    r = _region(meta, BoundingBox([0] * nd, bound), 1, False, 0, [0] * nd)
    rows = [_u64(x, nd) for x in rows]
    B = rows[0].shape[0]
    wave_of = np.zeros(max(B, 1), np.uint32)
    n = getattr(L, name)(ctypes.byref(r), *[x.ctypes.data for x in rows], B, wave_of.ctypes.data)
    return int(n), [int(w) for w in wave_of[:B]]


def regions_waves(meta: ArrayMetadata, offsets, shape: Sequence[int]):
    """zcg_regions_waves (host code, no GPU): the greedy split of the boxes
    `offsets` (B x ndim) of one `shape` into consecutive runs of pairwise
    disjoint boxes -> (number of waves, wave index per box).  scatter_regions
    calls for the waves, in order on one stream, let the later box win."""
    return _waves("zcg_regions_waves", meta, shape, offsets)


def write_ndarrays(hier, path_name: str, meta: ArrayMetadata, offsets, arrays, device: int = 0,
                   slot_budget_bytes: int = 0, flags: int = 0, shape: Sequence[int] = None) -> None:
    """write_ndarray for many boxes of one shape in one native call
    (zcg_store_write_boxes[_device]): the store ends up as if write_ndarray had
    run for offsets[0], offsets[1], ... in that order (a later box wins where
    two overlap), but every chunk the boxes touch is read at most once, and
    encoded and written once.  `arrays` is a numpy array of shape (B, *shape),
    or a uint8 device tensor holding the B boxes back to back, each dense in
    the chunk memory order — what read_ndarrays(..., as_tensor=True) returns,
    so a read / modify / write round trip needs no host copy; a flat tensor
    does not say the box shape, which `shape` then gives.  `flags`: decode
    flags for the chunks that are read first; `slot_budget_bytes` bounds the
    decoded chunks held on the device at a time (0: 4 GiB)."""
    tensor_in = not isinstance(arrays, np.ndarray) and hasattr(arrays, "data_ptr")
    nd = meta.get_ndim()
    if tensor_in:
        tensor = arrays
        if shape is None:
            raise ZarrIOError("InvalidInput", "a device tensor of boxes needs the box shape")
        shape = [int(x) for x in shape]
        if len(shape) != nd:
            raise ZarrIOError("InvalidData", "Wrong number of dimensions")
        dt = np.dtype(meta.effective_type().numpy_dtype()).newbyteorder("=")
    else:
        arrays = np.asarray(arrays)
        if arrays.ndim != nd + 1:
            raise ZarrIOError("InvalidData", "Wrong number of dimensions")
        shape = [int(x) for x in arrays.shape[1:]]
        dt = arrays.dtype.newbyteorder("=")
    check_array_type(dt, meta)
    offs = _u64(offsets, nd)
    if not tensor_in and arrays.shape[0] != offs.shape[0]:
        raise ZarrIOError("InvalidData", "Bounding boxes and arrays differ in number")
    bx = _Boxes(meta, offs, [shape] * offs.shape[0], dt.itemsize)
    call = _StoreCall(hier, path_name, meta, flags, device)
    bshape = (ctypes.c_uint64 * _native.MAX_DIMS)(*shape)
    if tensor_in:
        if tensor.numel() * tensor.element_size() < bx.at[-1]:
            raise ZarrIOError("InvalidData", "Bounding boxes and array have different shape")
        ins = bx.pointers(tensor.data_ptr())
        istr = (ctypes.c_int64 * _native.MAX_DIMS)(*_strides(shape, bx.order))
        call("write_boxes", "zcg_store_write_boxes_device", ctypes.addressof(bshape), ctypes.addressof(istr),
             bx.offs.ctypes.data, ctypes.addressof(ins), bx.B, slot_budget_bytes, 16)
    else:
        # box b dense in the chunk memory order, the boxes back to back
        host = np.ascontiguousarray(arrays.astype(dt, copy=False).transpose([0] + list(range(nd, 0, -1)))
                                    if bx.order == "F" else arrays.astype(dt, copy=False))
        ins = bx.pointers(host.ctypes.data if host.size else 0)
        call("write_boxes", "zcg_store_write_boxes", ctypes.addressof(bshape), bx.offs.ctypes.data,
             ctypes.addressof(ins), bx.B, slot_budget_bytes, 16)


def vboxes_tensor(offsets, shapes, strides, bases, device: int = 0):
    """Device uint8 tensor of _native.VBox records (zcg_vbox): per box its
    offset, shape and view strides (elements) per array dim and the device
    address of element (0, ..., 0) of its view."""
    import torch
    B = len(offsets)
    arr = (_native.VBox * max(B, 1))()
    for b in range(B):
        for d in range(len(offsets[b])):
            arr[b].offset[d] = int(offsets[b][d])
            arr[b].shape[d] = int(shapes[b][d])
            arr[b].strides[d] = int(strides[b][d])
        arr[b].base = int(bases[b])
    raw = np.frombuffer(bytes(arr), np.uint8)[: B * ctypes.sizeof(_native.VBox)].copy()
    return torch.from_numpy(raw).to(torch.device("cuda", device))


def regions_v_scratch_bytes(n_boxes: int) -> int:
    """zcg_regions_v_scratch_bytes: device working memory of one _v call."""
    return int(_native.load_library().zcg_regions_v_scratch_bytes(int(n_boxes)))


def _regions_vs(record, scratch_bytes, name: str, meta: ArrayMetadata, bound, es, table, table_lo, table_n, boxes,
                status, scratch, fill, fill_value, device, stream) -> None:
    """The _v and _s device-level calls: `record` is the box record type
    (_native.VBox or SBox), `scratch_bytes` its call's scratch size function."""
    ctx = _native.context(device)
    nd = meta.get_ndim()
    r = _region(meta, BoundingBox([0] * nd, bound), es, fill, fill_value, [0] * nd)
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in table_lo])
    n = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in table_n])
    n_boxes = boxes.numel() * boxes.element_size() // ctypes.sizeof(record) if boxes is not None else 0
    if n_boxes and scratch is None:
        import torch
        scratch = torch.empty(scratch_bytes(n_boxes), dtype=torch.uint8, device=boxes.device)
    st = getattr(ctx.lib, name)(ctx.handle, ctypes.byref(r), ctypes.addressof(lo), ctypes.addressof(n),
                                table.data_ptr() if table is not None else None,
                                boxes.data_ptr() if n_boxes else None, n_boxes,
                                scratch.data_ptr() if scratch is not None else None,
                                status.data_ptr() if status is not None else None, _stream_handle(stream, device))
    _raise_status(st, ctx, name[4:])


def assemble_regions_v(meta: ArrayMetadata, bound: Sequence[int], es: int, table, table_lo, table_n, boxes, status,
                       fill: bool, fill_value: int, device: int = 0, stream=None, scratch=None) -> None:
    """Device-level call for many boxes of differing shapes
    (zcg_read_regions_v): assemble_regions with `boxes` = device tensor of
    _native.VBox records (vboxes_tensor), each with its own shape and view, and
    `bound` = the largest extent per dimension any box may have.  `scratch` =
    device tensor of regions_v_scratch_bytes(B) bytes (None: allocated here,
    which a captured call must not do).  Asynchronous."""
    _regions_vs(_native.VBox, regions_v_scratch_bytes, "zcg_read_regions_v", meta, bound, es, table, table_lo,
                table_n, boxes, status, scratch, fill, fill_value, device, stream)


def scatter_regions_v(meta: ArrayMetadata, bound: Sequence[int], es: int, table, table_lo, table_n, boxes, status,
                      device: int = 0, stream=None, scratch=None) -> None:
    """Device-level inverse of assemble_regions_v (zcg_write_regions_v): every
    box's view is written into the chunk slots of `table`.  Boxes of one call
    that overlap leave either value; split the call with regions_v_waves where
    the later box must win.  Asynchronous."""
    _regions_vs(_native.VBox, regions_v_scratch_bytes, "zcg_write_regions_v", meta, bound, es, table, table_lo,
                table_n, boxes, status, scratch, False, 0, device, stream)


def _bound(shapes, nd: int) -> List[int]:
    return [max([int(s[d]) for s in shapes] or [0]) for d in range(nd)]


def regions_v_grid(meta: ArrayMetadata, offsets, shapes):
    """zcg_regions_v_grid (host code, no GPU): the union of the boxes' grid
    ranges -> (lo, n)."""
    return _grid("zcg_regions_v_grid", meta, _bound(shapes, meta.get_ndim()), offsets, shapes)


def regions_v_waves(meta: ArrayMetadata, offsets, shapes):
    """zcg_regions_v_waves (host code, no GPU): regions_waves for boxes
    `offsets` (B x ndim) with `shapes` (B x ndim) -> (number of waves, wave
    index per box)."""
    return _waves("zcg_regions_v_waves", meta, _bound(shapes, meta.get_ndim()), offsets, shapes)


def _read_boxes(hier, path_name, meta, boxes, steps, t, device, as_tensor, flags, slot_budget_bytes):
    """read_ndarrays_v (steps None) and read_ndarrays_s."""
    check_array_type(t, meta)
    nd = meta.get_ndim()
    for bb in boxes:
        if len(bb.offset) != nd:
            raise ZarrIOError("InvalidData", "Wrong number of dimensions")
    stp = None if steps is None else _steps_arg(steps, len(boxes), nd)
    dt = np.dtype(t).newbyteorder("=")
    bx = _Boxes(meta, [bb.offset for bb in boxes], [bb.shape for bb in boxes], dt.itemsize, stp)
    call = _StoreCall(hier, path_name, meta, flags, device)
    buf, outs = bx.out(device if as_tensor else None)
    name = "zcg_store_read_boxes_" + ("v" if stp is None else "s") + ("_device" if as_tensor else "")
    args = [bx.shp.ctypes.data] + ([] if stp is None else [stp.ctypes.data]) + ([None, 1] if as_tensor else [])
    call("read_boxes", name, *args, bx.offs.ctypes.data, ctypes.addressof(outs), bx.B, slot_budget_bytes, 16)
    if as_tensor:
        return buf[: bx.at[-1]], bx.at[:-1], bx.strides
    return [v.copy(order=bx.order) for v in bx.views(buf, dt)]


def read_ndarrays_v(hier, path_name: str, meta: ArrayMetadata, boxes: Sequence[BoundingBox], t, device: int = 0,
                    as_tensor: bool = False, flags: int = 0, slot_budget_bytes: int = 0):
    """read_ndarray for many boxes of differing shapes in one native call
    (zcg_store_read_boxes_v[_device]): a list of arrays whose [b] equals
    read_ndarray(..., boxes[b], t).  The chunks the boxes share are read and
    decoded once.  With as_tensor the result is (uint8 device tensor of the
    boxes back to back, byte offset per box, element strides per box), each box
    dense in the chunk memory order."""
    return _read_boxes(hier, path_name, meta, boxes, None, t, device, as_tensor, flags, slot_budget_bytes)


def write_ndarrays_v(hier, path_name: str, meta: ArrayMetadata, offsets, arrays, device: int = 0,
                     slot_budget_bytes: int = 0, flags: int = 0) -> None:
    """write_ndarray for many boxes of differing shapes in one native call
    (zcg_store_write_boxes_v): `arrays` is a sequence of numpy arrays, box b
    written at offsets[b].  The store ends up as if write_ndarray had run for
    box 0, 1, ... in that order (a later box wins where two overlap), but every
    chunk the boxes touch is read at most once, and encoded and written once.
    `flags`: decode flags for the chunks that are read first."""
    arrays = list(arrays)
    offs = _u64(offsets, meta.get_ndim())
    B = offs.shape[0]
    if len(arrays) != B:
        raise ZarrIOError("InvalidData", "Bounding boxes and arrays differ in number")
    dense, shp, ins = _dense_inputs(meta, arrays)
    _StoreCall(hier, path_name, meta, flags, device)(
        "write_boxes", "zcg_store_write_boxes_v", shp.ctypes.data, offs.ctypes.data, ctypes.addressof(ins), B,
        slot_budget_bytes, 16)


def sboxes_tensor(offsets, shapes, steps, strides, bases, device: int = 0):
    """Device uint8 tensor of _native.SBox records (zcg_sbox): per box its
    offset, sample counts, steps and view strides (elements) per array dim and
    the device address of element (0, ..., 0) of its view."""
    import torch
    B = len(offsets)
    arr = (_native.SBox * max(B, 1))()
    for b in range(B):
        for d in range(len(offsets[b])):
            arr[b].offset[d] = int(offsets[b][d])
            arr[b].shape[d] = int(shapes[b][d])
            arr[b].step[d] = int(steps[b][d])
            arr[b].strides[d] = int(strides[b][d])
        arr[b].base = int(bases[b])
    raw = np.frombuffer(bytes(arr), np.uint8)[: B * ctypes.sizeof(_native.SBox)].copy()
    return torch.from_numpy(raw).to(torch.device("cuda", device))


def regions_s_scratch_bytes(n_boxes: int) -> int:
    """zcg_regions_s_scratch_bytes: device working memory of one _s call."""
    return int(_native.load_library().zcg_regions_s_scratch_bytes(int(n_boxes)))


def regions_s_grid(meta: ArrayMetadata, offsets, shapes, steps):
    """zcg_regions_s_grid (host code, no GPU): the union of the grid ranges of
    the boxes' hulls (`shapes`: sample counts, `steps`: B x ndim) -> (lo, n)."""
    return _grid("zcg_regions_s_grid", meta, _bound(shapes, meta.get_ndim()), offsets, shapes, steps)


def region_s_chunks(meta: ArrayMetadata, offset, shape, step, want_touched: bool = True):
    """zcg_region_s_chunks (host code, no GPU) for one strided box -> (lo, n,
    touched, count): the hull's grid range, per dimension a list of n[d] 0/1
    flags (1: grid index lo[d] + j holds a sample; None without want_touched),
    and the number of touched chunks (the product of the touched counts)."""
    L = _native.load_library()
    nd = meta.get_ndim()
    r = _region(meta, BoundingBox([0] * nd, [0] * nd), 1, False, 0, [0] * nd)
    off = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in offset])
    shp = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in shape])
    stp = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in step])
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)()
    n = (ctypes.c_uint64 * _native.MAX_DIMS)()
    args = (ctypes.byref(r), ctypes.addressof(off), ctypes.addressof(shp), ctypes.addressof(stp),
            ctypes.addressof(lo), ctypes.addressof(n))
    count = int(L.zcg_region_s_chunks(*args, None))
    lo_l, n_l = [int(lo[d]) for d in range(nd)], [int(n[d]) for d in range(nd)]
    if not want_touched:
        return lo_l, n_l, None, count
    flags = np.zeros(max(sum(n_l), 1), np.uint8)
    count = int(L.zcg_region_s_chunks(*args, flags.ctypes.data))
    at = np.concatenate([[0], np.cumsum(n_l)]).astype(int)
    return lo_l, n_l, [flags[at[d]:at[d + 1]].tolist() for d in range(nd)], count


def assemble_regions_s(meta: ArrayMetadata, bound: Sequence[int], es: int, table, table_lo, table_n, boxes, status,
                       fill: bool, fill_value: int, device: int = 0, stream=None, scratch=None) -> None:
    """Device-level call for many strided boxes (zcg_read_regions_s):
    assemble_regions_v with `boxes` = device tensor of _native.SBox records
    (sboxes_tensor), each with its own sample counts, steps and view, and
    `bound` = the largest sample count per dimension any box may have.  Table
    entries of chunks that hold no sample are never read.  `scratch` = device
    tensor of regions_s_scratch_bytes(B) bytes (None: allocated here, which a
    captured call must not do).  Asynchronous."""
    _regions_vs(_native.SBox, regions_s_scratch_bytes, "zcg_read_regions_s", meta, bound, es, table, table_lo,
                table_n, boxes, status, scratch, fill, fill_value, device, stream)


def scatter_regions_s(meta: ArrayMetadata, bound: Sequence[int], es: int, table, table_lo, table_n, boxes, status,
                      scratch=None, device: int = 0, stream=None) -> None:
    """Device-level inverse of assemble_regions_s (zcg_write_regions_s): sample
    i of every box's view is written to array index offset + i * step in the
    chunk slots of `table`, and no other byte of a slot is.  Table entries of
    chunks that hold no sample are never read.  Boxes of one call that share a
    sample leave either value; split the call with regions_s_waves where the
    later box must win.  `scratch` as for assemble_regions_s.  Asynchronous."""
    _regions_vs(_native.SBox, regions_s_scratch_bytes, "zcg_write_regions_s", meta, bound, es, table, table_lo,
                table_n, boxes, status, scratch, False, 0, device, stream)


def regions_s_waves(meta: ArrayMetadata, offsets, shapes, steps):
    """zcg_regions_s_waves (host code, no GPU): regions_v_waves for strided
    boxes (`shapes`: sample counts, `steps`: B x ndim) -> (number of waves,
    wave index per box).  Two boxes intersect only where they share a sample,
    so interleaved boxes (even and odd planes) stay in one wave."""
    return _waves("zcg_regions_s_waves", meta, [0] * meta.get_ndim(), offsets, shapes, steps)


def _steps_arg(steps, B: int, nd: int) -> np.ndarray:
    """`steps` as a B x ndim uint64 array: one step vector for all boxes, or one
    per box; every step >= 1."""
    try:
        a = np.array(steps, dtype=object)
        if a.ndim == 1 and a.shape[0] == nd:
            a = np.broadcast_to(a, (B, nd))
        if a.shape != (B, nd):
            raise ValueError
        vals = [[int(x) for x in row] for row in a]
    except (ValueError, TypeError):
        raise ZarrIOError("InvalidInput", f"steps must hold {nd} entries, or {B} x {nd}") from None
    if any(x < 1 for row in vals for x in row):
        raise ZarrIOError("InvalidInput", "every step must be at least 1")
    return np.ascontiguousarray(np.array(vals, dtype=np.uint64).reshape(B, nd))


def read_ndarrays_s(hier, path_name: str, meta: ArrayMetadata, boxes: Sequence[BoundingBox], steps, t,
                    device: int = 0, as_tensor: bool = False, flags: int = 0, slot_budget_bytes: int = 0):
    """read_ndarray for many strided boxes in one native call
    (zcg_store_read_boxes_s[_device]): boxes[b].shape is the number of samples,
    sample i along d is array index offset[d] + i * step[d]; `steps` is B x ndim,
    or one step vector for all boxes.  The result is a list of arrays whose [b]
    equals read_ndarray(..., hull_b, t)[::step], where hull_b is the dense box
    offset .. offset + (shape - 1) * step + 1.  Only the chunks that hold a
    sample are read and decoded, each once.  With as_tensor the result is what
    read_ndarrays_v returns: (uint8 device tensor of the boxes back to back,
    byte offset per box, element strides per box)."""
    return _read_boxes(hier, path_name, meta, boxes, steps, t, device, as_tensor, flags, slot_budget_bytes)


def _check_hulls(meta: ArrayMetadata, shp: np.ndarray, stp: np.ndarray) -> None:
    """The native calls' limit, raised before a context is needed: positions in
    a hull are 32-bit."""
    for b in range(shp.shape[0]):
        for d, cs in enumerate(meta.chunk_shape):
            c, k = int(shp[b, d]), int(stp[b, d])
            if c > 1 and (c - 1) * k + int(cs) >= 1 << 32:
                raise ZarrIOError("Unsupported", f"box {b}: hull extent + chunk extent along a dimension must stay "
                                                 "below 2^32")


def write_ndarrays_s(hier, path_name: str, meta: ArrayMetadata, offsets, steps, arrays, device: int = 0,
                     slot_budget_bytes: int = 0, flags: int = 0) -> None:
    """a[offset::step] = array for many boxes in one native call
    (zcg_store_write_boxes_s[_device]): element i of arrays[b] along d goes to
    array index offsets[b][d] + i * step[d]; `steps` is B x ndim, or one step
    vector for all boxes, and an array's shape is its box's sample counts.  The
    store ends up as if, box by box in order, the hull had been read, the
    samples overlaid and the hull's touched chunks written (a later box wins a
    shared sample), but only the chunks that hold a sample are read, encoded
    and written, each once.  `arrays` is a sequence of numpy arrays (the host
    call) or of device tensors (the device call; any strides, the dtype's item
    size must be the array's).  `flags`: decode flags for the chunks that are
    read first."""
    nd = meta.get_ndim()
    arrays = list(arrays)
    offs = _u64(offsets, nd)
    B = offs.shape[0]
    if len(arrays) != B:
        raise ZarrIOError("InvalidData", "Bounding boxes and arrays differ in number")
    stp = _steps_arg(steps, B, nd)
    tensor_in = B > 0 and all(not isinstance(a, np.ndarray) and hasattr(a, "data_ptr") for a in arrays)
    if tensor_in:
        dt = np.dtype(meta.effective_type().numpy_dtype()).newbyteorder("=")
        check_array_type(dt, meta)
        for a in arrays:
            if a.dim() != nd:
                raise ZarrIOError("InvalidData", "Wrong number of dimensions")
            if a.element_size() != dt.itemsize:
                raise ZarrIOError("InvalidData", "Tensor and array differ in their element size")
        shp = _u64([list(a.shape) for a in arrays], nd)
        istr = np.ascontiguousarray(np.array([list(a.stride()) for a in arrays], dtype=np.int64).reshape(-1, nd))
        ins = (ctypes.c_void_p * max(B, 1))(*[a.data_ptr() for a in arrays])
        name, views = "zcg_store_write_boxes_s_device", [istr.ctypes.data]
    else:
        dense, shp, ins = _dense_inputs(meta, arrays)
        name, views = "zcg_store_write_boxes_s", []
    _check_hulls(meta, shp, stp)
    _StoreCall(hier, path_name, meta, flags, device)(
        "write_boxes", name, shp.ctypes.data, stp.ctypes.data, *views, offs.ctypes.data, ctypes.addressof(ins), B,
        slot_budget_bytes, 16)


def read_ndarray_into(hier, path_name: str, meta: ArrayMetadata, bbox: BoundingBox, arr: np.ndarray, t,
                      device: int = 0, flags: int = 0) -> None:
    """ZarrNdarrayReader::read_ndarray_into (ndarray.rs:176-268): elements
    that no present chunk covers keep their values; `arr` may be any
    writable view of the box's shape."""
    import torch
    check_array_type(t, meta)
    if len(bbox.offset) != meta.get_ndim() or meta.get_ndim() != arr.ndim:
        raise ZarrIOError("InvalidData", "Wrong number of dimensions")
    if list(arr.shape) != list(bbox.shape):
        raise ZarrIOError("InvalidData", "Bounding box and array have different shape")
    dt = np.dtype(t).newbyteorder("=")
    es = dt.itemsize
    staged = np.ascontiguousarray(arr, dtype=dt)
    st = _strides(bbox.shape, "C")
    dev = torch.device("cuda", device)
    out = torch.from_numpy(staged.reshape(-1).view(np.uint8).copy() if staged.size else np.zeros(1, np.uint8)).to(dev)
    table, keep = _decode_visited(hier, path_name, meta, bbox, device, flags)
    assemble_region(meta, bbox, es, table, out, st, False, 0, device)
    torch.cuda.synchronize(device)
    if staged.size:
        np.copyto(arr, out.cpu().numpy().view(dt).reshape(staged.shape))


def write_ndarray(hier, path_name: str, meta: ArrayMetadata, offset: Sequence[int], array: np.ndarray,
                  device: int = 0) -> None:
    """ZarrNdarrayWriter::write_ndarray (ndarray.rs:276-385) on the GPU: the
    chunks the box touches are read and decoded when only partly covered
    (absent ones start as fill value), the box is scattered into them by
    zcg_write_region, and all of them are encoded in one batch and written
    through the store's set() semantics (filesystem.rs:260-280)."""
    import torch
    if array.ndim != meta.get_ndim():
        raise ZarrIOError("InvalidData", "Wrong number of dimensions")
    dt = array.dtype.newbyteorder("=")
    check_array_type(dt, meta)
    es = dt.itemsize
    bbox = BoundingBox(offset, list(array.shape))
    lo, n = region_grid(meta, bbox)
    coords = list(itertools.product(*[range(l, l + k) for l, k in zip(lo, n)]))  # C order
    if not coords or bbox.is_empty():
        return
    cs = meta.get_chunk_shape()
    N = meta.get_chunk_num_elements()
    D = N * es
    dev = torch.device("cuda", device)
    codec = BatchCodec(device)
    cap = codec.encode_bound(meta, D)
    box = torch.from_numpy(np.ascontiguousarray(array, dtype=dt).reshape(-1).view(np.uint8).copy()).to(dev)
    per = max(1, WRITE_BATCH_BYTES // max(D + cap, 1))
    for b0 in range(0, len(coords), per):
        _write_sub_batch(hier, path_name, meta, bbox, coords, b0, min(len(coords), b0 + per), dt, D, N, cap,
                         box, device, dev)


def _write_sub_batch(hier, path_name, meta, bbox, coords, b0, b1, dt, D, N, cap, box, device, dev):
    """write_ndarray for coords[b0:b1]: read/decode the partly covered chunks
    into their slots (store get(): shared flock), scatter the box into all of
    them, encode and write every chunk file through the store's set()
    (zcg_store_write_chunks_device: exclusive flock, then truncate)."""
    import torch
    from .storage import store_read_device, store_write_device
    cs = meta.get_chunk_shape()
    m = b1 - b0
    slots = torch.empty(m * D, dtype=torch.uint8, device=dev)
    ptrs = [slots.data_ptr() + i * D for i in range(m)]
    paths = [hier.chunk_path(path_name, meta, coords[b0 + i]) for i in range(m)]
    partial = []
    for i in range(m):
        c = coords[b0 + i]
        assert meta.in_bounds(c)  # storage.rs:217
        nom = BoundingBox([ci * s for ci, s in zip(c, cs)], cs)
        wb = BoundingBox(nom.offset, nom.shape)
        wb.intersect(bbox)
        if wb != nom:
            partial.append(i)  # fully overwritten chunks are not read (ndarray.rs:328-337)
    absent = []
    if partial:
        st = store_read_device(meta, [paths[i] for i in partial], [ptrs[i] for i in partial], device)
        for k, i in enumerate(partial):
            if st[k] == _native.ABSENT:
                absent.append(i)  # starts as fill value (ndarray.rs:357-368)
            elif st[k] != _native.OK:
                raise ZarrIOError(_native.STATUS_NAMES.get(int(st[k]), str(st[k])), f"chunk {list(coords[b0 + i])}")
    if absent:
        fill = np.full(N, 0 if meta.fill_value is None else meta.fill_value, dtype=dt)
        ft = torch.from_numpy(fill.view(np.uint8)).to(dev)
        for i in absent:
            slots[i * D:(i + 1) * D].copy_(ft)
    # the region call covers the whole grid range: chunks outside this
    # sub-batch get NULL slots and are skipped
    table_h = np.zeros(len(coords), np.int64)
    table_h[b0:b1] = ptrs
    table = torch.from_numpy(table_h).to(dev)
    scatter_region(meta, bbox, dt.itemsize, table, box, _strides(bbox.shape, "C"), device)
    torch.cuda.synchronize(dev)  # the store's streams read the slots next
    st = store_write_device(meta, paths, ptrs, device)
    bad = np.nonzero(st != 0)[0]
    if len(bad):
        i = int(bad[0])
        raise ZarrIOError(_native.STATUS_NAMES.get(int(st[i]), str(st[i])), f"chunk {list(coords[b0 + i])}")


# ---- a list of coordinates (numpy's a[i, j, k] with index arrays) -------------

def _coords_arg(coords, nd: int) -> np.ndarray:
    """`coords` as a contiguous (P, ndim) uint64 array: a (P, ndim) integer
    array, or a tuple of ndim index arrays as numpy's a[i, j, k] takes."""
    if isinstance(coords, tuple):
        if len(coords) != nd:
            raise ZarrIOError("InvalidData", "Wrong number of dimensions")
        cols = [np.asarray(c).reshape(-1) for c in coords]
        if len({c.shape[0] for c in cols}) > 1:
            raise ValueError("index arrays differ in length")
        a = np.stack(cols, axis=1) if cols[0].shape[0] else np.zeros((0, nd), np.uint64)
    else:
        a = np.asarray(coords)
        if a.size == 0:
            a = np.zeros((0, nd), np.uint64)
        if a.ndim != 2 or a.shape[1] != nd:
            raise ZarrIOError("InvalidData", "Wrong number of dimensions")
    if a.dtype.kind not in "iu" and a.dtype != object:
        raise TypeError("coordinates must be integers")
    if a.size and (a.dtype.kind == "i" or a.dtype == object) and min(int(x) for x in a.reshape(-1)) < 0:
        raise ValueError("negative coordinate")
    return np.ascontiguousarray(a.astype(np.uint64))


def points_grid(meta: ArrayMetadata, coords):
    """zcg_points_grid (host code, no GPU): the smallest grid range that holds
    every chunk a point visits -> (lo, n); regions_v_grid with shapes all 1."""
    nd = meta.get_ndim()
    return _grid("zcg_points_grid", meta, [1] * nd, _coords_arg(coords, nd))


def points_last(coords) -> np.ndarray:
    """zcg_points_last (host code, no GPU): a bool array, True where no later
    point has the same coordinate.  `coords` is (P, ndim)."""
    L = _native.load_library()
    a = np.asarray(coords)
    c = _coords_arg(coords, len(coords) if isinstance(coords, tuple) else (a.shape[1] if a.ndim == 2 else 1))
    keep = np.zeros(max(c.shape[0], 1), np.uint8)
    L.zcg_points_last(c.ctypes.data, c.shape[0], c.shape[1], keep.ctypes.data)
    return keep[: c.shape[0]].astype(bool)


def _points(name: str, meta: ArrayMetadata, es, table, table_lo, table_n, coords, vals, first_outside, fill,
            fill_value, device, stream) -> None:
    ctx = _native.context(device)
    nd = meta.get_ndim()
    r = _region(meta, BoundingBox([0] * nd, [1] * nd), es, fill, fill_value, [0] * nd)
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in table_lo])
    n = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in table_n])
    P = coords.numel() * coords.element_size() // (8 * nd) if coords is not None else 0
    st = getattr(ctx.lib, name)(ctx.handle, ctypes.byref(r), ctypes.addressof(lo), ctypes.addressof(n),
                                table.data_ptr() if table is not None else None,
                                coords.data_ptr() if P else None, P,
                                vals.data_ptr() if vals is not None else None,
                                first_outside.data_ptr() if first_outside is not None else None,
                                _stream_handle(stream, device))
    _raise_status(st, ctx, name[4:])


def assemble_points(meta: ArrayMetadata, es: int, table, table_lo, table_n, coords, out, first_outside,
                    fill: bool = False, fill_value: int = 0, device: int = 0, stream=None) -> None:
    """Device-level gather (zcg_read_points): `coords` = device int64/uint64
    tensor of P x ndim coordinates, `out` = dense device tensor of P elements,
    `first_outside` = device tensor of one 64-bit word (UINT64_MAX, or the
    lowest index of a point whose chunk lies outside the table).  The table
    arguments are assemble_regions'.  Asynchronous."""
    _points("zcg_read_points", meta, es, table, table_lo, table_n, coords, out, first_outside, fill, fill_value,
            device, stream)


def scatter_points(meta: ArrayMetadata, es: int, table, table_lo, table_n, coords, values, first_outside,
                   device: int = 0, stream=None) -> None:
    """Device-level inverse of assemble_points (zcg_write_points): value i goes
    to the chunk slot element of point i.  Points of one call that share a
    coordinate leave either value; drop the earlier ones with points_last where
    the later one must win.  Asynchronous."""
    _points("zcg_write_points", meta, es, table, table_lo, table_n, coords, values, first_outside, False, 0,
            device, stream)


def read_points(hier, path_name: str, meta: ArrayMetadata, coords, t, device: int = 0, as_tensor: bool = False,
                slot_budget_bytes: int = 0, io_threads: int = 0, flags: int = 0):
    """a[coords] in one native call (zcg_store_read_points[_device]): a 1-D
    array (with as_tensor a device tensor) of len(coords) elements, element i
    being read_ndarray of the 1-element box at coords[i].  Only the chunks that
    hold a point are opened, each decoded once."""
    import torch
    check_array_type(t, meta)
    nd = meta.get_ndim()
    c = _coords_arg(coords, nd)
    P = c.shape[0]
    dt = np.dtype(t).newbyteorder("=")
    call = _StoreCall(hier, path_name, meta, flags, device)
    threads = io_threads or 16
    if as_tensor:
        out = torch.empty(max(P, 1) * dt.itemsize, dtype=torch.uint8, device=torch.device("cuda", device))
        call("read_points", "zcg_store_read_points_device", c.ctypes.data, P, 1, out.data_ptr(), slot_budget_bytes,
             threads)
        return out[: P * dt.itemsize].view(getattr(torch, dt.name)) if hasattr(torch, dt.name) else out[: P * dt.itemsize]
    host = np.empty(max(P, 1), dt)
    call("read_points", "zcg_store_read_points", c.ctypes.data, P, host.ctypes.data, slot_budget_bytes, threads)
    return host[:P]


def write_points(hier, path_name: str, meta: ArrayMetadata, coords, values, device: int = 0,
                 slot_budget_bytes: int = 0, io_threads: int = 0, flags: int = 0) -> None:
    """a[coords] = values in one native call (zcg_store_write_points[_device]):
    the store ends up as if write_ndarray had run for the 1-element boxes in
    order, so of two points with one coordinate the later one wins.  `values`
    is a numpy array, or a device tensor, of len(coords) elements.  Every chunk
    that holds a point is read at most once, and encoded and written once.
    `flags`: decode flags for the chunks that are read first."""
    nd = meta.get_ndim()
    c = _coords_arg(coords, nd)
    P = c.shape[0]
    call = _StoreCall(hier, path_name, meta, flags, device)
    threads = io_threads or 16
    if hasattr(values, "data_ptr"):
        if values.numel() != P:
            raise ZarrIOError("InvalidData", "Coordinates and values differ in number")
        v = values.contiguous()
        if v.element_size() != call.am.array.dtype.elem_size:
            raise ZarrIOError("InvalidData", "Element size differs from the array's")
        call("write_points", "zcg_store_write_points_device", c.ctypes.data, P, v.data_ptr(), slot_budget_bytes,
             threads)
    else:
        a = np.asarray(values).reshape(-1)
        if a.shape[0] != P:
            raise ZarrIOError("InvalidData", "Coordinates and values differ in number")
        dt = a.dtype.newbyteorder("=")
        check_array_type(dt, meta)
        a = np.ascontiguousarray(a.astype(dt, copy=False))
        call("write_points", "zcg_store_write_points", c.ctypes.data, P, a.ctypes.data if P else None,
             slot_budget_bytes, threads)


# ---- an orthogonal selection (numpy's a[np.ix_(rows, cols, planes)], zarr's oindex) ----

def _sel_arg(sel, shape: Sequence[int]) -> List[np.ndarray]:
    """`sel` as one contiguous uint64 index array per dimension.  An entry is an
    integer array or list; a slice, resolved against the dimension's extent as
    numpy does (a negative step is just a list); a boolean array of the
    dimension's length, taken as flatnonzero; or an int, an axis of length 1
    that is kept."""
    sel = list(sel) if isinstance(sel, (tuple, list)) else [sel]
    if len(sel) != len(shape):
        raise ZarrIOError("InvalidData", "Wrong number of dimensions")
    lists = []
    for d, s in enumerate(sel):
        if isinstance(s, slice):
            a = np.arange(*s.indices(int(shape[d])), dtype=np.int64)
        elif isinstance(s, (bool, np.bool_)):
            raise TypeError("a selection entry must be integers, a slice or a boolean array")
        elif isinstance(s, (int, np.integer)):
            a = np.array([int(s)], dtype=object)
        else:
            a = np.asarray(s)
            if a.dtype == bool:
                if a.ndim != 1 or a.shape[0] != int(shape[d]):
                    raise IndexError(f"boolean selection along dimension {d} has length {a.shape[0] if a.ndim else 0}, "
                                     f"the dimension has {int(shape[d])}")
                a = np.flatnonzero(a)
            elif a.size == 0:
                a = np.zeros(0, np.uint64)
            a = a.reshape(-1)
        if a.dtype.kind not in "iu" and a.dtype != object:
            raise TypeError("a selection entry must be integers, a slice or a boolean array")
        if a.size and (a.dtype.kind == "i" or a.dtype == object) and min(int(x) for x in a) < 0:
            raise ValueError(f"negative index along dimension {d}")
        lists.append(np.ascontiguousarray(a.astype(np.uint64)))
    return lists


def _list_pointers(lists):
    """(pointer array, count array) over host index arrays or device tensors."""
    ptrs = (ctypes.c_void_p * _native.MAX_DIMS)(*[(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
                                                  if _numel(a) else None for a in lists])
    counts = (ctypes.c_uint64 * _native.MAX_DIMS)(*[_numel(a) for a in lists])
    return ptrs, counts


def _numel(a) -> int:
    return int(a.size) if isinstance(a, np.ndarray) else int(a.numel())


def ortho_scratch_bytes(counts: Sequence[int]) -> int:
    """zcg_ortho_scratch_bytes: device working memory of one ortho call."""
    c = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in counts])
    return int(_native.load_library().zcg_ortho_scratch_bytes(len(counts), ctypes.addressof(c)))


def ortho_chunks(meta: ArrayMetadata, sel, want_touched: bool = True):
    """zcg_ortho_chunks (host code, no GPU) -> (lo, n, touched, count): the
    smallest grid range that holds every visited chunk, per dimension a list of
    n[d] 0/1 flags (1: grid index lo[d] + j holds a visiting index of the
    dimension's list; None without want_touched), and the number of touched
    chunks (the product of the touched counts)."""
    L = _native.load_library()
    nd = meta.get_ndim()
    lists = _sel_arg(sel, meta.shape)
    r = _region(meta, BoundingBox([0] * nd, [1] * nd), 1, False, 0, [0] * nd)
    ptrs, counts = _list_pointers(lists)
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)()
    n = (ctypes.c_uint64 * _native.MAX_DIMS)()
    args = (ctypes.byref(r), ctypes.addressof(ptrs), ctypes.addressof(counts), ctypes.addressof(lo),
            ctypes.addressof(n))
    count = int(L.zcg_ortho_chunks(*args, None))
    lo_l, n_l = [int(lo[d]) for d in range(nd)], [int(n[d]) for d in range(nd)]
    if not want_touched:
        return lo_l, n_l, None, count
    flags = np.zeros(max(sum(n_l), 1), np.uint8)
    count = int(L.zcg_ortho_chunks(*args, flags.ctypes.data))
    at = np.concatenate([[0], np.cumsum(n_l)]).astype(int)
    return lo_l, n_l, [flags[at[d]:at[d + 1]].tolist() for d in range(nd)], count


def _ortho(name: str, meta: ArrayMetadata, es, table, table_lo, table_n, lists, view, strides, outside, fill,
           fill_value, device, stream, scratch) -> None:
    ctx = _native.context(device)
    nd = meta.get_ndim()
    if len(lists) != nd:
        raise ZarrIOError("InvalidData", "Wrong number of dimensions")
    r = _region(meta, BoundingBox([0] * nd, [1] * nd), es, fill, fill_value, [0] * nd)
    lo = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in table_lo])
    n = (ctypes.c_uint64 * _native.MAX_DIMS)(*[int(x) for x in table_n])
    sel = _native.OSel()
    for d in range(nd):
        sel.count[d] = _numel(lists[d])
        sel.index[d] = lists[d].data_ptr() if sel.count[d] else None
        sel.strides[d] = int(strides[d])
    sel.base = view.data_ptr() if view is not None else None
    if scratch is None and all(sel.count[d] for d in range(nd)):
        import torch
        scratch = torch.empty(ortho_scratch_bytes([sel.count[d] for d in range(nd)]), dtype=torch.uint8,
                              device=view.device)
    st = getattr(ctx.lib, name)(ctx.handle, ctypes.byref(r), ctypes.addressof(lo), ctypes.addressof(n),
                                table.data_ptr() if table is not None else None, ctypes.addressof(sel),
                                scratch.data_ptr() if scratch is not None else None,
                                outside.data_ptr() if outside is not None else None, _stream_handle(stream, device))
    _raise_status(st, ctx, name[4:])


def assemble_ortho(meta: ArrayMetadata, es: int, table, table_lo, table_n, lists, out, out_strides, outside,
                   fill: bool = False, fill_value: int = 0, device: int = 0, stream=None, scratch=None) -> None:
    """Device-level gather of an orthogonal selection (zcg_read_ortho): `lists`
    = one device int64/uint64 tensor of array indices per dimension, `out` =
    device tensor whose data_ptr() is element (0, ..., 0) of a view with
    `out_strides` (elements, per array dimension), `outside` = device tensor of
    ndim 64-bit words (per dimension UINT64_MAX, or the lowest position in the
    list whose chunk lies outside the table).  Element (i_0, .., i_{n-1}) is what
    assemble_points gives the point (lists[0][i_0], .., lists[n-1][i_{n-1}]).
    `scratch` = device tensor of ortho_scratch_bytes(counts) bytes (None:
    allocated here, which a captured call must not do).  Asynchronous."""
    _ortho("zcg_read_ortho", meta, es, table, table_lo, table_n, lists, out, out_strides, outside, fill, fill_value,
           device, stream, scratch)


def scatter_ortho(meta: ArrayMetadata, es: int, table, table_lo, table_n, lists, values, value_strides, outside,
                  device: int = 0, stream=None, scratch=None) -> None:
    """Device-level inverse of assemble_ortho (zcg_write_ortho): element
    (i_0, .., i_{n-1}) of the view goes to the chunk slot element of its point.
    With duplicate indices in a list one value wins whole; drop the earlier
    duplicates per list with points_last where the later one must win.
    Asynchronous."""
    _ortho("zcg_write_ortho", meta, es, table, table_lo, table_n, lists, values, value_strides, outside, False, 0,
           device, stream, scratch)


def read_ortho(hier, path_name: str, meta: ArrayMetadata, sel, t, device: int = 0, as_tensor: bool = False,
               slot_budget_bytes: int = 0, io_threads: int = 0, flags: int = 0):
    """a[np.ix_(*sel)] in one native call (zcg_store_read_ortho[_device]): an
    array (with as_tensor a device tensor) whose shape is the lengths of the
    selection's lists, element (i_0, .., i_{n-1}) being read_points at
    (sel[0][i_0], .., sel[n-1][i_{n-1}]).  `sel` holds one entry per dimension
    (_sel_arg).  Only the touched chunks, the product of the per-dimension
    touched grid indices, are opened, each decoded once."""
    import torch
    check_array_type(t, meta)
    lists = _sel_arg(sel, meta.shape)
    counts = [int(a.size) for a in lists]
    total = int(np.prod(counts, dtype=object))
    dt = np.dtype(t).newbyteorder("=")
    call = _StoreCall(hier, path_name, meta, flags, device)
    threads = io_threads or 16
    ptrs, cnt = _list_pointers(lists)
    if as_tensor:
        out = torch.empty(max(total, 1) * dt.itemsize, dtype=torch.uint8, device=torch.device("cuda", device))
        call("read_ortho", "zcg_store_read_ortho_device", ctypes.addressof(ptrs), ctypes.addressof(cnt), 1,
             out.data_ptr(), slot_budget_bytes, threads)
        out = out[: total * dt.itemsize]
        return out.view(getattr(torch, dt.name)).reshape(counts) if hasattr(torch, dt.name) else out
    host = np.empty(max(total, 1), dt)
    call("read_ortho", "zcg_store_read_ortho", ctypes.addressof(ptrs), ctypes.addressof(cnt), host.ctypes.data,
         slot_budget_bytes, threads)
    return host[:total].reshape(counts)


def write_ortho(hier, path_name: str, meta: ArrayMetadata, sel, values, device: int = 0,
                slot_budget_bytes: int = 0, io_threads: int = 0, flags: int = 0) -> None:
    """a[np.ix_(*sel)] = values in one native call
    (zcg_store_write_ortho[_device]): the store ends up as after write_points
    on the product of the lists in C order, so per list the last occurrence of
    an index wins.  `values` is a numpy array, or a device tensor, of the
    selection's shape.  Every touched chunk is read at most once (not at all
    where the selection covers it), and encoded and written once.  `flags`:
    decode flags for the chunks that are read first."""
    lists = _sel_arg(sel, meta.shape)
    counts = [int(a.size) for a in lists]
    total = int(np.prod(counts, dtype=object))
    call = _StoreCall(hier, path_name, meta, flags, device)
    threads = io_threads or 16
    ptrs, cnt = _list_pointers(lists)
    if hasattr(values, "data_ptr"):
        if values.numel() != total:
            raise ZarrIOError("InvalidData", "Selection and values differ in number")
        v = values.contiguous()
        if v.element_size() != call.am.array.dtype.elem_size:
            raise ZarrIOError("InvalidData", "Element size differs from the array's")
        call("write_ortho", "zcg_store_write_ortho_device", ctypes.addressof(ptrs), ctypes.addressof(cnt),
             v.data_ptr(), slot_budget_bytes, threads)
    else:
        a = np.asarray(values)
        if a.size != total:
            raise ZarrIOError("InvalidData", "Selection and values differ in number")
        dt = a.dtype.newbyteorder("=")
        check_array_type(dt, meta)
        a = np.ascontiguousarray(a.astype(dt, copy=False)).reshape(-1)
        call("write_ortho", "zcg_store_write_ortho", ctypes.addressof(ptrs), ctypes.addressof(cnt),
             a.ctypes.data if total else None, slot_budget_bytes, threads)
