"""Device-resident bulk path on torch tensors (torch = device memory + streams only).

`Engine` wraps lz4f_mi355x_engine; tensors are uint8 CUDA(HIP) tensors whose data_ptr() goes straight
into the C ABI.  Work is enqueued on torch's current stream, so torch.cuda.Event timings bracket it.
"""
from __future__ import annotations

import ctypes
import weakref

import numpy as np
import torch

from . import _ffi
from ._ffi import Block, FrameInfo, Preferences, Result, TrainParams


class DeviceCodecError(Exception):
    pass


def _chk(L, r):
    if L.LZ4F_isError(r):
        raise DeviceCodecError("%s (%s)" % (L.LZ4F_getErrorName(r).decode(), L.lz4f_mi355x_last_error().decode()))
    return r


def _check_batch_args(src, src_off, dst, dst_off, results, rec_bytes: int) -> int:
    """The tensors of a batch call (Engine.decompress_frames_async) -> the number of frames; ValueError for what is wrong with them."""
    for name, t, dt in (("src", src, torch.uint8), ("dst", dst, torch.uint8), ("src_off", src_off, torch.int64), ("dst_off", dst_off, torch.int64),
                        ("results", results, torch.uint8)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a tensor" % name)
        if t.dtype != dt:
            raise ValueError("%s must be %s, not %s" % (name, dt, t.dtype))
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous 1-d tensor" % name)
    if src_off.numel() < 1 or src_off.numel() != dst_off.numel():
        raise ValueError("src_off and dst_off must both hold n+1 offsets (got %d and %d)" % (src_off.numel(), dst_off.numel()))
    n = src_off.numel() - 1
    if n >= 1 << 32:
        raise ValueError("too many frames for one call")
    if results.numel() < n * rec_bytes:
        raise ValueError("results must hold %d bytes for %d frames (got %d)" % (n * rec_bytes, n, results.numel()))
    if not all(t.is_cuda for t in (src, dst, src_off, dst_off, results)):
        raise ValueError("the tensors of a batch must be in device memory")
    if len({src.device, dst.device, src_off.device, dst_off.device, results.device}) != 1:
        raise ValueError("the tensors of a batch must be on one device")
    return n


def _check_measure_args(src, src_off, results, dst_off, rec_bytes: int) -> int:
    """The tensors of a measure call (Engine.measure_frames_async) -> the number of frames; ValueError for what is wrong with them."""
    named = [("src", src, torch.uint8), ("src_off", src_off, torch.int64), ("results", results, torch.uint8)]
    if dst_off is not None:
        named.append(("dst_off", dst_off, torch.int64))
    for name, t, dt in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a tensor" % name)
        if t.dtype != dt:
            raise ValueError("%s must be %s, not %s" % (name, dt, t.dtype))
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous 1-d tensor" % name)
    if src_off.numel() < 1:
        raise ValueError("src_off must hold n+1 offsets (got %d)" % src_off.numel())
    if dst_off is not None and dst_off.numel() != src_off.numel():
        raise ValueError("src_off and dst_off must both hold n+1 offsets (got %d and %d)" % (src_off.numel(), dst_off.numel()))
    n = src_off.numel() - 1
    if n >= 1 << 32:
        raise ValueError("too many frames for one call")
    if results.numel() < n * rec_bytes:
        raise ValueError("results must hold %d bytes for %d frames (got %d)" % (n * rec_bytes, n, results.numel()))
    if not all(t.is_cuda for _, t, _ in named):
        raise ValueError("the tensors of a batch must be in device memory")
    if len({t.device for _, t, _ in named}) != 1:
        raise ValueError("the tensors of a batch must be on one device")
    return n


def _check_tensors(named, what: str = "a batch") -> None:
    """(name, tensor, dtype) triples: contiguous 1-d device tensors of those types on one device; ValueError otherwise."""
    for name, t, dt in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s must be a tensor" % name)
        if t.dtype != dt:
            raise ValueError("%s must be %s, not %s" % (name, dt, t.dtype))
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous 1-d tensor" % name)
    if not all(t.is_cuda for _, t, _ in named):
        raise ValueError("the tensors of %s must be in device memory" % what)
    if len({t.device for _, t, _ in named}) != 1:
        raise ValueError("the tensors of %s must be on one device" % what)


def _check_pack_args(src, src_off, results, dst, dst_off, record, rec_bytes: int) -> int:
    """The tensors of a pack call (Engine.pack_frames_async) -> the number of frames; ValueError for what is wrong with them."""
    named = [("src", src, torch.uint8), ("src_off", src_off, torch.int64), ("results", results, torch.uint8), ("dst", dst, torch.uint8),
             ("dst_off", dst_off, torch.int64)]
    if record is not None:
        named.append(("record", record, torch.uint8))
    _check_tensors(named)
    if src_off.numel() < 1 or src_off.numel() != dst_off.numel():
        raise ValueError("src_off and dst_off must both hold n+1 offsets (got %d and %d)" % (src_off.numel(), dst_off.numel()))
    n = src_off.numel() - 1
    if n >= 1 << 32:
        raise ValueError("too many frames for one call")
    if results.numel() < n * rec_bytes:
        raise ValueError("results must hold %d bytes for %d frames (got %d)" % (n * rec_bytes, n, results.numel()))
    if record is not None and record.numel() < rec_bytes:
        raise ValueError("record must hold %d bytes (got %d)" % (rec_bytes, record.numel()))
    return n


def _check_read_directory_args(pack, n_frames, src_off, record, rec_bytes: int) -> int:
    """The arguments of Engine.read_pack_directory_async -> the number of frames; ValueError for what is wrong with them."""
    named = [("pack", pack, torch.uint8), ("src_off", src_off, torch.int64)]
    if record is not None:
        named.append(("record", record, torch.uint8))
    _check_tensors(named, "a directory read")
    if not isinstance(n_frames, int) or isinstance(n_frames, bool) or not 0 <= n_frames < 1 << 32:
        raise ValueError("n_frames must be an int in [0, 2^32)")
    if src_off.numel() != n_frames + 1:
        raise ValueError("src_off must hold n_frames+1 = %d offsets (got %d)" % (n_frames + 1, src_off.numel()))
    if record is not None and record.numel() < rec_bytes:
        raise ValueError("record must hold %d bytes (got %d)" % (rec_bytes, record.numel()))
    return n_frames


def _check_split_args(src, max_frames, src_off, record, rec_bytes: int) -> int:
    """The arguments of Engine.split_frames_async -> max_frames; ValueError for what is wrong with them."""
    named = [("src", src, torch.uint8), ("src_off", src_off, torch.int64)]
    if record is not None:
        named.append(("record", record, torch.uint8))
    _check_tensors(named, "a split")
    if not isinstance(max_frames, int) or isinstance(max_frames, bool) or not 0 <= max_frames < 1 << 32:
        raise ValueError("max_frames must be an int in [0, 2^32)")
    if src_off.numel() != max_frames + 1:
        raise ValueError("src_off must hold max_frames+1 = %d offsets (got %d)" % (max_frames + 1, src_off.numel()))
    if record is not None and record.numel() < rec_bytes:
        raise ValueError("record must hold %d bytes (got %d)" % (rec_bytes, record.numel()))
    return max_frames


def _check_train_args(src, src_off, dict_out, params, record, rec_bytes: int) -> int:
    """The arguments of Engine.train_dict_async -> the number of samples; ValueError for what is wrong with them."""
    named = [("src", src, torch.uint8), ("src_off", src_off, torch.int64), ("dict_out", dict_out, torch.uint8)]
    if record is not None:
        named.append(("record", record, torch.uint8))
    _check_tensors(named, "a training call")
    if src_off.numel() < 1:
        raise ValueError("src_off must hold n+1 offsets (got %d)" % src_off.numel())
    n = src_off.numel() - 1
    if n >= 1 << 32:
        raise ValueError("too many samples for one call")
    if params is not None and not isinstance(params, TrainParams):
        raise ValueError("params must be a TrainParams (or None for the defaults)")
    if dict_out.numel() > 65536:
        raise ValueError("dict_out must hold at most 65536 bytes (got %d): LZ4 never reads further back" % dict_out.numel())
    if record is not None and record.numel() < rec_bytes:
        raise ValueError("record must hold %d bytes (got %d)" % (rec_bytes, record.numel()))
    return n


TRAIN_TILE = 4096       # LZ4F_MI355X_TRAIN_TILE: the corpus positions a workgroup of the training kernels takes at a time (for tests and tools)
TRAIN_SCAN_TILE = 1024  # LZ4F_MI355X_TRAIN_SCAN_TILE: the samples a step of the offsets' scan takes
TRAIN_DEFAULTS = {"k": 64, "d": 8, "f": 18, "rounds": 16}      # LZ4F_MI355X_TRAIN_K, _D, _F, _ROUNDS
PACK_TILE = 16384       # LZ4F_MI355X_PACK_TILE: the output bytes a workgroup of the pack's copy kernel takes at a time (for tests and tools)
PACK_DIRECTORY = 0x1    # LZ4F_MI355X_PACK_DIRECTORY


def pack_directory_size(n: int) -> int:
    """The bytes of a packed stream's frame directory for n frames (24 + 4 n).  Host arithmetic only: no device is touched."""
    if not isinstance(n, int) or isinstance(n, bool) or not 0 <= n < 1 << 32:
        raise ValueError("n must be an int in [0, 2^32)")
    return int(_ffi.lib().lz4f_mi355x_packDirectorySize(n))


def peek_pack_directory(head: bytes) -> "tuple[int, int, int]":
    """The fixed part of a packed stream's directory, from its first 24 bytes in host memory -> (directory bytes, n_frames, frames
    bytes): the stream is directory bytes + frames bytes long, and Engine.read_pack_directory_async wants that n_frames.
    DeviceCodecError (frameHeader_incomplete, frameType_unknown, frameSize_wrong) for what is not such a head."""
    if not isinstance(head, (bytes, bytearray, memoryview)):
        raise ValueError("head must be bytes")
    head = bytes(head)
    L = _ffi.lib()
    n, fb = ctypes.c_uint32(0), ctypes.c_uint64(0)
    d = _chk(L, L.lz4f_mi355x_peekPackDirectory(head, len(head), ctypes.byref(n), ctypes.byref(fb)))
    return int(d), int(n.value), int(fb.value)


def frame_windows(lengths, prefs: Preferences, gap: int = 0) -> "list[int]":
    """Window offsets for Engine.compress_frames_async: n+1 cumulative offsets, window i being
    lz4f_mi355x_compressFrameBound(lengths[i], prefs) bytes - which always suffice for input i's frame - plus `gap` spare bytes
    behind it.  Host arithmetic only: no device is touched."""
    if not isinstance(prefs, Preferences):
        raise ValueError("prefs must be a Preferences")
    if gap < 0:
        raise ValueError("gap must not be negative")
    L = _ffi.lib()
    offs = [0]
    for n in lengths:
        offs.append(offs[-1] + _chk(L, L.lz4f_mi355x_compressFrameBound(int(n), ctypes.byref(prefs))) + gap)
    return offs


class CDict:
    """A prepared dictionary (Engine.create_cdict): the engine's own copy of the dictionary's last 64 KiB in device memory and the
    match finder's table digested from it once.  It serves any number of compress_frames_async(..., cdict=) calls on the engine that
    made it, and decompress_frames_async(..., dictionary=) takes it too.  close() waits for the engine's stream and frees it; the
    engine closes the ones that are still open when it is closed itself.  Use it as a context manager to close it on the way out.
    One made with create_cdict(..., hc=True) also carries the hash-chain finder's digest and serves compression levels 3-12 (`hc`)."""

    def __init__(self, engine: "Engine", h):
        self.engine, self.h = engine, h
        n = ctypes.c_size_t(0)
        p = engine.L.lz4f_mi355x_cdict_data(h, ctypes.byref(n))
        self.data_ptr, self.size = (p or None), int(n.value)

    @property
    def hc(self) -> bool:
        """Whether it carries the hash-chain finder's digest (create_cdict(..., hc=True)); False once closed."""
        return bool(self.h) and bool(self.engine.L.lz4f_mi355x_cdict_has_hc(self.h))

    def close(self):
        if self.h:
            for s in [s for s in list(self.engine._dictsets) if any(m is self for m in s.members)]:      # (the sets that borrow it go first)
                s.close()
            h, self.h = self.h, None
            self.data_ptr, self.size = None, 0
            self.engine._cdicts.discard(self)
            self.engine.L.lz4f_mi355x_dev_freeCDict(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


DICT_NONE = 0xFFFFFFFF        # LZ4F_MI355X_DICT_NONE: a slot's "this frame has no dictionary"
DICT_UNKNOWN = 0xFFFFFFFE     # LZ4F_MI355X_DICT_UNKNOWN: resolve_dict_ids_async's "the header names an ID the set does not have"
PATH_DICT_UNKNOWN = 0x4000    # LZ4F_MI355X_PATH_DICT_UNKNOWN: the path bit (flags >> 12) of a frame that failed because its slot is no member


class DictSet:
    """A set of prepared dictionaries (Engine.create_dictset): member k is a CDict of the same engine (None: a dictionary of no bytes)
    with the ID dict_ids[k].  compress_frames_async / decompress_frames_async(..., dictset=, slots=) then give every frame of a batch
    its own member - by slots, an int32 device tensor of member indexes (DICT_NONE, as -1: no dictionary), or, decoding with
    slots=None, by the dictID in each frame's header.  The members are borrowed: the set keeps references to them, and must be
    closed before they are (the engine closes its sets first).  close() waits for the engine's stream and frees the set's table."""

    def __init__(self, engine: "Engine", h, members, dict_ids):
        self.engine, self.h = engine, h
        self.members, self.dict_ids = tuple(members), tuple(dict_ids)

    def __len__(self) -> int:
        return int(self.engine.L.lz4f_mi355x_dictset_count(self.h)) if self.h else 0

    def close(self):
        if self.h:
            h, self.h = self.h, None
            self.engine._dictsets.discard(self)
            self.engine.L.lz4f_mi355x_dev_freeDictSet(h)
            self.members = ()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    def __init__(self, device: int = 0, stream: "torch.cuda.Stream | None" = None):
        self.L = _ffi.lib()
        self.device = device
        torch.cuda.set_device(device)
        self.stream = stream if stream is not None else torch.cuda.current_stream(device)
        h = ctypes.c_void_p()
        _chk(self.L, self.L.lz4f_mi355x_engine_create(ctypes.byref(h), device, ctypes.c_void_p(self.stream.cuda_stream), 1))
        self.h = h
        self._cdicts = weakref.WeakSet()                                          # the prepared dictionaries still open: closed with the engine
        self._dictsets = weakref.WeakSet()                                        # the dictionary sets still open: closed before the CDicts
        self._res = torch.zeros(32, dtype=torch.uint8, device="cuda:%d" % device)
        self._res_host = torch.zeros(32, dtype=torch.uint8).pin_memory()      # the result record comes back by DMA into page-locked memory: one wait, no staging

    def close(self):
        if self.h:
            for s in list(self._dictsets):                                        # (a set is freed before its members)
                s.close()
            for c in list(self._cdicts):                                          # (a CDict is freed before its engine)
                c.close()
            self.L.lz4f_mi355x_engine_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    TIMING_SLOTS = ("find_matches", "layout", "emit", "xxh32_write", "walk", "xxh32_verify", "decode", "finish", "decode_parse", "decode_copy", "compress_total", "decompress_total")

    def set_deterministic(self, on: bool):
        """Equal input -> equal bytes (one wave per workgroup parses, in order); about a tenth of the match finder's speed."""
        _chk(self.L, self.L.lz4f_mi355x_engine_set_deterministic(self.h, 1 if on else 0))

    def set_timing(self, on: bool):
        _chk(self.L, self.L.lz4f_mi355x_engine_set_timing(self.h, 1 if on else 0))

    def get_timing(self) -> dict:
        ms = (ctypes.c_float * len(self.TIMING_SLOTS))()
        _chk(self.L, self.L.lz4f_mi355x_engine_get_timing_n(self.h, ms, len(self.TIMING_SLOTS)))
        return dict(zip(self.TIMING_SLOTS, [float(x) for x in ms]))

    # -- helpers
    def _result(self) -> Result:
        with torch.cuda.stream(self.stream):
            self._res_host.copy_(self._res, non_blocking=True)
        self.stream.synchronize()
        return Result.from_buffer_copy(self._res_host.numpy().tobytes())

    def frame_bound(self, n: int, prefs: Preferences) -> int:
        return _chk(self.L, self.L.lz4f_mi355x_compressFrameBound(n, ctypes.byref(prefs)))

    INBAND = (1 << 64) - 1

    def frame_bound_inband(self, n: int, prefs: Preferences) -> int:
        """Room for a frame with its trailer (block list + sequence index in a skippable frame behind it)."""
        return self.frame_bound(n, prefs) + int(self.L.lz4f_mi355x_trailer_bound(n, ctypes.byref(prefs)))

    def compress_async(self, src: torch.Tensor, dst: torch.Tensor, prefs: Preferences, table: "torch.Tensor | None" = None,
                       index: "torch.Tensor | None" = None, inband: bool = False):
        """Enqueue src -> one frame in dst.  prefs.compressionLevel picks the encoder: <= 2 the fast one, 3-12 the
        high-compression levels (hash-chain search, lazy parse; equal input -> equal bytes at any setting), above 12 is 12.
        Returns nothing; call result() after a sync.
        With `index` (new_index) the compressor also leaves its sequence index there for decompress_blocks_async.
        With `inband` the index and the block list go into the stream itself (a skippable frame behind the LZ4 frame, counted in
        result().size): decompress_frame_async finds them there."""
        assert src.dtype == torch.uint8 and dst.dtype == torch.uint8 and src.is_cuda and dst.is_cuda
        if inband:
            _chk(self.L, self.L.lz4f_mi355x_dev_compressFrameIndexed(self.h, dst.data_ptr(), dst.numel(), src.data_ptr(), src.numel(), ctypes.byref(prefs),
                                                                    self._res.data_ptr(), table.data_ptr() if table is not None else None, None, self.INBAND))
            return
        if index is not None:
            assert table is not None and index.dtype == torch.uint8 and index.is_cuda
            _chk(self.L, self.L.lz4f_mi355x_dev_compressFrameIndexed(self.h, dst.data_ptr(), dst.numel(), src.data_ptr(), src.numel(), ctypes.byref(prefs),
                                                                    self._res.data_ptr(), table.data_ptr(), index.data_ptr(), index.numel()))
            return
        _chk(self.L, self.L.lz4f_mi355x_dev_compressFrame(self.h, dst.data_ptr(), dst.numel(), src.data_ptr(), src.numel(), ctypes.byref(prefs),
                                                         self._res.data_ptr(), table.data_ptr() if table is not None else None))

    def decompress_blocks_async(self, frame: torch.Tensor, frame_len: int, dst: torch.Tensor, table: torch.Tensor, n_blocks: int, info: FrameInfo,
                                index: "torch.Tensor | None" = None):
        if index is not None:
            _chk(self.L, self.L.lz4f_mi355x_dev_decompressBlocksIndexed(self.h, dst.data_ptr(), dst.numel(), frame.data_ptr(), frame_len, table.data_ptr(),
                                                                       n_blocks, ctypes.byref(info), index.data_ptr(), index.numel(), self._res.data_ptr()))
            return
        _chk(self.L, self.L.lz4f_mi355x_dev_decompressBlocks(self.h, dst.data_ptr(), dst.numel(), frame.data_ptr(), frame_len, table.data_ptr(),
                                                            n_blocks, ctypes.byref(info), self._res.data_ptr()))

    def decompress_frame_async(self, frame: torch.Tensor, frame_len: int, dst: torch.Tensor):
        _chk(self.L, self.L.lz4f_mi355x_dev_decompressFrame(self.h, dst.data_ptr(), dst.numel(), frame.data_ptr(), frame_len, self._res.data_ptr()))

    RESULT_BYTES = ctypes.sizeof(Result)

    def new_results(self, n: int) -> torch.Tensor:
        """Room for the result records of a batch of n frames (decompress_frames_async)."""
        return torch.zeros(n * self.RESULT_BYTES, dtype=torch.uint8, device="cuda:%d" % self.device)

    def _check_dictionary(self, dictionary) -> "tuple[int | None, int]":
        """A batch call's dictionary: a uint8 tensor on the engine's device (one dimension, contiguous; it may be empty)."""
        if (not isinstance(dictionary, torch.Tensor) or dictionary.dtype != torch.uint8 or not dictionary.is_cuda or dictionary.dim() != 1
                or not dictionary.is_contiguous() or dictionary.device.index != self.device):
            raise ValueError("dictionary must be a contiguous one-dimensional uint8 tensor on cuda:%d" % self.device)
        return (dictionary.data_ptr() if dictionary.numel() else None), dictionary.numel()

    def create_cdict(self, dictionary: torch.Tensor, hc: bool = False) -> CDict:
        """Prepare a dictionary (a uint8 tensor on the engine's device; it may be empty) for compress_frames_async(..., cdict=): its
        last 64 KiB are copied and digested on the engine's stream, once.  The tensor may be reused or freed once the stream has run
        the call; nothing is read back.  hc=True also digests it for the hash-chain finder (one more kernel, up to 144 KiB more
        device memory): the CDict then serves compression levels 3-12 too, and is the plain one at levels 0-2."""
        d_ptr, d_len = self._check_dictionary(dictionary)
        h = ctypes.c_void_p()
        create = self.L.lz4f_mi355x_dev_createCDictHC if hc else self.L.lz4f_mi355x_dev_createCDict
        _chk(self.L, create(self.h, ctypes.byref(h), d_ptr, d_len))
        c = CDict(self, h)
        self._cdicts.add(c)
        return c

    def _check_cdict(self, cdict) -> CDict:
        if not isinstance(cdict, CDict) or cdict.h is None:
            raise ValueError("cdict must be an open CDict (Engine.create_cdict)")
        return cdict

    def create_dictset(self, cdicts, dict_ids) -> DictSet:
        """A set of this engine's CDicts (None: a member of no bytes), member k under the ID dict_ids[k] (ints in [0, 2^32), pairwise
        distinct; at most 65 536 members, an empty set is valid).  One small table goes to the device on the engine's stream;
        nothing is read back."""
        cdicts, dict_ids = list(cdicts), list(dict_ids)
        if len(cdicts) != len(dict_ids):
            raise ValueError("cdicts and dict_ids must be equally long (got %d and %d)" % (len(cdicts), len(dict_ids)))
        for c in cdicts:
            if c is not None: self._check_cdict(c)
        for i in dict_ids:
            if not isinstance(i, int) or isinstance(i, bool) or not 0 <= i < 1 << 32:
                raise ValueError("a dictID must be an int in [0, 2^32)")
        n = len(cdicts)
        hs = (ctypes.c_void_p * max(n, 1))(*[c.h if c is not None else None for c in cdicts])
        ids = (ctypes.c_uint32 * max(n, 1))(*dict_ids)
        h = ctypes.c_void_p()
        _chk(self.L, self.L.lz4f_mi355x_dev_createDictSet(self.h, ctypes.byref(h), n, hs, ids))
        s = DictSet(self, h, cdicts, dict_ids)
        self._dictsets.add(s)
        return s

    def _check_dictset(self, dictset, slots, n: int, others, need_slots: bool) -> "int | None":
        """A set call's dictset= and slots= -> slots' address (None: by the headers).  slots: an int32 device tensor of n elements."""
        if not isinstance(dictset, DictSet) or dictset.h is None:
            raise ValueError("dictset must be an open DictSet (Engine.create_dictset)")
        if slots is None:
            if need_slots:
                raise ValueError("slots must be given with dictset=")
            return None
        _check_tensors(list(others) + [("slots", slots, torch.int32)])
        if slots.numel() != n:
            raise ValueError("slots must hold one element per frame: %d (got %d)" % (n, slots.numel()))
        return slots.data_ptr()

    def resolve_dict_ids_async(self, src: torch.Tensor, src_off: torch.Tensor, dictset: DictSet, slots: torch.Tensor):
        """Enqueue the lookup of every frame's dictID in the set: slots (int32 device tensor of n elements) receives, for the first
        frame in src[src_off[i]:src_off[i+1]], the member whose ID the header names, DICT_NONE (-1 as int32) for a frame without the
        field, a skippable frame, a header that does not parse or a span outside src, and DICT_UNKNOWN (-2) for an ID that no member
        has - what decompress_frames_async(..., dictset=, slots=None) uses, to look at or to change before decoding.  Nothing is read
        back: no synchronisation."""
        named = [("src", src, torch.uint8), ("src_off", src_off, torch.int64)]
        _check_tensors(named)
        if src_off.numel() < 1:
            raise ValueError("src_off must hold n+1 offsets (got %d)" % src_off.numel())
        n = src_off.numel() - 1
        if n >= 1 << 32:
            raise ValueError("too many frames for one call")
        p = self._check_dictset(dictset, slots, n, named, True)
        _chk(self.L, self.L.lz4f_mi355x_dev_resolveDictIDs(self.h, n, src.data_ptr(), src.numel(), src_off.data_ptr(), dictset.h, p))

    def decompress_frames_async(self, src: torch.Tensor, src_off: torch.Tensor, dst: torch.Tensor, dst_off: torch.Tensor, results: torch.Tensor,
                                dictionary: "torch.Tensor | CDict | None" = None, dictset: "DictSet | None" = None,
                                slots: "torch.Tensor | None" = None):
        """Enqueue a batch: frame i is the first frame in src[src_off[i]:src_off[i+1]], its output goes to dst[dst_off[i]:dst_off[i+1]].
        src, dst: uint8 device tensors; src_off, dst_off: int64 device tensors of n+1 offsets; results: uint8 device tensor of
        32*n bytes (new_results).  Each frame's verdict lands in its record (frame_results) - a bad frame fails alone, the call
        raises only for what is wrong with the call itself.  Nothing is read back: no synchronisation.
        dictionary (a uint8 tensor on the engine's device): one shared dictionary for the whole batch, as LZ4F_decompress_usingDict
        applies it - the history in front of every frame (linked blocks) or every block (independent blocks); its last 64 KiB count.
        It must stay alive until the stream has run the call.  The header's dictID is not looked at.  A CDict (create_cdict) is
        taken too: the dictionary is then its own copy.
        dictset (create_dictset; not together with dictionary=): a dictionary per frame - frame i decodes with the member slots[i]
        (int32 device tensor of n elements; DICT_NONE, -1: none), or with slots=None the member whose ID its own header names (no
        dictID field: none).  A slot or an ID that is no member fails that frame alone (ERROR_GENERIC, PATH_DICT_UNKNOWN in its
        record's path bits) and leaves its window untouched."""
        n = _check_batch_args(src, src_off, dst, dst_off, results, self.RESULT_BYTES)
        call, tail = self.L.lz4f_mi355x_dev_decompressFrames, ()
        if dictset is not None:
            if dictionary is not None:
                raise ValueError("give dictionary= or dictset=, not both")
            p = self._check_dictset(dictset, slots, n, [("src", src, torch.uint8)], False)
            call, tail = self.L.lz4f_mi355x_dev_decompressFrames_usingDictSet, (dictset.h, p)
        elif slots is not None:
            raise ValueError("slots= goes with dictset=")
        elif dictionary is not None:
            call = self.L.lz4f_mi355x_dev_decompressFrames_usingDict
            if isinstance(dictionary, CDict):
                tail = (self._check_cdict(dictionary).data_ptr, dictionary.size)
            else:
                tail = self._check_dictionary(dictionary)
        _chk(self.L, call(self.h, n, src.data_ptr(), src.numel(), src_off.data_ptr(), dst.data_ptr(), dst.numel(), dst_off.data_ptr(), results.data_ptr(), *tail))

    def measure_frames_async(self, src: torch.Tensor, src_off: torch.Tensor, results: torch.Tensor, dst_off: "torch.Tensor | None" = None):
        """Enqueue a measurement: what frame i, the first frame in src[src_off[i]:src_off[i+1]], decodes to - its size from the tokens,
        consumed, n_blocks and flags as decompress_frames_async reports them - lands in its record; nothing is decoded and nothing
        else written.  dst_off (int64 device tensor of n+1 elements, optional) receives the offsets of windows that
        decompress_frames_async accepts for these frames, the total in dst_off[n]: a frame of short flushed blocks needs more than its
        size, a frame that fails gets an empty window.  Match offsets and checksums are not looked at: the decode may still reject a
        frame for those.  Nothing is read back: no synchronisation.  The pipeline for frames of unknown size, on one stream:

            eng.measure_frames_async(src, src_off, results, dst_off)
            dst = torch.empty(capacity, dtype=torch.uint8, device=src.device)      # capacity >= dst_off[-1] (the one read-back, if there is no bound)
            eng.decompress_frames_async(src, src_off, dst, dst_off, results)"""
        n = _check_measure_args(src, src_off, results, dst_off, self.RESULT_BYTES)
        _chk(self.L, self.L.lz4f_mi355x_dev_measureFrames(self.h, n, src.data_ptr(), src.numel(), src_off.data_ptr(),
                                                         dst_off.data_ptr() if dst_off is not None else None, results.data_ptr()))

    def compress_frames_async(self, src: torch.Tensor, src_off: torch.Tensor, dst: torch.Tensor, dst_off: torch.Tensor, prefs: Preferences,
                              results: torch.Tensor, dictionary: "torch.Tensor | None" = None, cdict: "CDict | None" = None,
                              dictset: "DictSet | None" = None, slots: "torch.Tensor | None" = None):
        """Enqueue a batch: input i is src[src_off[i]:src_off[i+1]], its frame is written at dst[dst_off[i]] and may use
        dst[dst_off[i]:dst_off[i+1]] (this module's frame_windows gives offsets that always suffice).  One prefs for all frames; a non-zero
        prefs.frameInfo.contentSize means every header declares its own input's length.  Tensors as for decompress_frames_async,
        whose src / src_off the dst / dst_off of this call can be as they are.  Each frame is byte for byte what compress_async
        writes for its input alone on an engine with set_deterministic(True); its size and verdict land in its record
        (frame_results) - a frame whose window is too small fails alone.  Nothing is read back: no synchronisation.
        dictionary (a uint8 tensor on the engine's device): one shared dictionary for the whole batch - the match finder reaches into
        its last 64 KiB as if they lay in front of every input; decompress_frames_async(..., dictionary=) and liblz4's
        LZ4F_decompress_usingDict decode the frames.  Levels 0-2 only (3-12 raise compressionLevel_invalid: there a dictionary comes
        as a CDict made with hc=True); prefs.frameInfo.dictID is written as it is and means nothing else.
        cdict (create_cdict, of this engine; not together with dictionary=): the same dictionary prepared once - the same frames,
        byte for byte, without reading and seeding the dictionary again for every 64 KiB chunk of every call.  Levels 3-12 take a
        CDict made with create_cdict(..., hc=True) - the hash-chain search with the dictionary in front of every frame or independent
        block - and raise compressionLevel_invalid for one made without.
        dictset with slots (create_dictset; not together with dictionary= or cdict=): a dictionary per frame - frame i is what cdict=
        the member slots[i] gives it alone, with that member's ID as the header's dictID (int32 device tensor of n elements;
        DICT_NONE, -1: the plain frame with prefs as they are).  A slot that is no member fails that frame alone.  Levels 3-12 want
        every non-empty member made with hc=True."""
        if not isinstance(prefs, Preferences):
            raise ValueError("prefs must be a Preferences")
        if (cdict is not None) + (dictionary is not None) + (dictset is not None) > 1:
            raise ValueError("give dictionary=, cdict= or dictset=, not more than one" if dictset is not None else "give dictionary= or cdict=, not both")
        n = _check_batch_args(src, src_off, dst, dst_off, results, self.RESULT_BYTES)
        call, tail = self.L.lz4f_mi355x_dev_compressFrames, ()
        if dictset is not None:
            p = self._check_dictset(dictset, slots, n, [("src", src, torch.uint8)], True)
            call, tail = self.L.lz4f_mi355x_dev_compressFrames_usingDictSet, (dictset.h, p)
        elif slots is not None:
            raise ValueError("slots= goes with dictset=")
        elif cdict is not None:
            call, tail = self.L.lz4f_mi355x_dev_compressFrames_usingCDict, (self._check_cdict(cdict).h,)
        elif dictionary is not None:
            call, tail = self.L.lz4f_mi355x_dev_compressFrames_usingDict, self._check_dictionary(dictionary)
        _chk(self.L, call(self.h, n, src.data_ptr(), src.numel(), src_off.data_ptr(), dst.data_ptr(), dst.numel(), dst_off.data_ptr(), ctypes.byref(prefs),
                          results.data_ptr(), *tail))

    def pack_frames_async(self, src: torch.Tensor, src_off: torch.Tensor, results: torch.Tensor, dst: torch.Tensor, dst_off: torch.Tensor,
                          directory: bool = False, record: "torch.Tensor | None" = None):
        """Enqueue the compaction of a batch, behind compress_frames_async on the same stream: src, src_off and results are that
        call's dst, dst_off and results as they are; the frames come to lie back to back in dst, frame i at dst[dst_off[i]:dst_off[i+1]]
        (dst_off: int64 device tensor of n+1 elements, written here).  No frame byte is parsed: frame i is results[i].size bytes when
        its record says status 0 and size and offsets hold (src_off[i] <= src_off[i+1] <= src.numel(), size within the window), and an
        empty span otherwise - slot i stays frame i, and the batch decoder reports frameHeader_incomplete for it.
        directory=True puts the frame directory in front (a skippable frame of pack_directory_size(n) bytes, which every LZ4 reader
        steps over): dst_off[0] is then its size, and a receiver needs nothing but the stream (read_pack_directory_async).
        dst[:dst_off[n]] with dst_off is what measure_frames_async and decompress_frames_async take as src and src_off, and what
        `lz4 -d` decodes to the inputs in order.  dst must not overlap src (DeviceCodecError; nothing is enqueued).
        record (uint8 device tensor of 32 bytes, optional) receives one Result: size = dst_off[n], consumed = the frames' bytes,
        n_blocks = the non-empty frames, first_bad_block = the first record with status 0 whose size or offsets lie (0xFFFFFFFF:
        none), status dstMaxSize_tooSmall when dst is smaller than dst_off[n] (dst is then untouched; dst_off and size say what was
        needed) or srcSize_tooLarge when the directory cannot say a frame's length (> 0xFFFFFFFF).  Nothing is read back: no
        synchronisation.  On one stream:

            eng.compress_frames_async(inp, inp_off, win, win_off, prefs, results, cdict=cd)
            eng.pack_frames_async(win, win_off, results, out, out_off, directory=True, record=rec)
            # send out[:size] - size is Result.from_buffer_copy(rec.cpu().numpy().tobytes()).size, the one read-back"""
        n = _check_pack_args(src, src_off, results, dst, dst_off, record, self.RESULT_BYTES)
        _chk(self.L, self.L.lz4f_mi355x_dev_packFrames(self.h, n, src.data_ptr(), src.numel(), src_off.data_ptr(), results.data_ptr(), dst.data_ptr(),
                                                      dst.numel(), dst_off.data_ptr(), PACK_DIRECTORY if directory else 0,
                                                      record.data_ptr() if record is not None else None))

    def read_pack_directory_async(self, pack: torch.Tensor, n_frames: int, src_off: torch.Tensor, record: "torch.Tensor | None" = None):
        """Enqueue the reading of a packed stream's directory (pack_frames_async(directory=True)): pack is the stream, a uint8 device
        tensor; n_frames what peek_pack_directory said of its head; src_off (int64 device tensor of n_frames+1 elements) receives
        the frames' offsets into pack, as measure_frames_async and decompress_frames_async take them.  Everything is checked on the
        device, every read bounded by pack.numel(): magic, tag and sizes, the stored n_frames against the argument, the lengths' sum
        against the stated frames bytes, and the whole stream against pack.numel().  A directory that fails gives n_frames+1 zeros -
        every span empty, every frame frameHeader_incomplete to the decoder - and its status in record (uint8 device tensor of 32
        bytes, optional: status, size = frames bytes, consumed = the stream's bytes, n_blocks = n_frames).  Nothing is read back.
        On one stream, with the head of the message on the host:

            d, n, fb = peek_pack_directory(head24)
            eng.read_pack_directory_async(pack, n, src_off)
            eng.measure_frames_async(pack, src_off, results, dst_off)
            eng.decompress_frames_async(pack, src_off, dst, dst_off, results)"""
        n = _check_read_directory_args(pack, n_frames, src_off, record, self.RESULT_BYTES)
        _chk(self.L, self.L.lz4f_mi355x_dev_readPackDirectory(self.h, n, pack.data_ptr(), pack.numel(), src_off.data_ptr(),
                                                             record.data_ptr() if record is not None else None))

    def split_frames_async(self, src: torch.Tensor, max_frames: int, src_off: torch.Tensor, record: "torch.Tensor | None" = None):
        """Enqueue the search for the frame boundaries of a concatenated LZ4 stream that came without a directory: src is the stream,
        a uint8 device tensor; src_off (int64 device tensor of max_frames+1 elements) receives the frames' offsets into src, as
        measure_frames_async and decompress_frames_async take them.  The answer is the serial walk's - skippable frames stepped over,
        LZ4 frames listed until something that is neither, or src's end - found without its chain of dependent reads: every position
        is looked at once, and the frames are the candidates reachable from position 0, so a .lz4 file inside a stored block or a
        skippable frame is never listed.  Span i runs to the next frame's first byte (the skippable frames behind frame i are in it);
        skippable frames in front of the first frame are in no span; surplus slots are empty spans (frameHeader_incomplete to the
        decoder).  No payload is parsed, no checksum verified.
        record (uint8 device tensor of 32 bytes, optional) receives one Result: status (the walk's: 0, or why it stopped;
        dstMaxSize_tooSmall when it ended well with more than max_frames frames), consumed = where the walk ended, n_blocks = all
        the frames found, size = their bytes, first_bad_block = the frames before an error's stop (0xFFFFFFFF: none), flags bit 8 =
        a skippable frame was stepped over.  Nothing is read back: no synchronisation.  On one stream:

            eng.split_frames_async(stream, max_frames, src_off, record=rec)
            eng.measure_frames_async(stream, src_off, results, dst_off)
            eng.decompress_frames_async(stream, src_off, dst, dst_off, results)"""
        n = _check_split_args(src, max_frames, src_off, record, self.RESULT_BYTES)
        _chk(self.L, self.L.lz4f_mi355x_dev_splitFrames(self.h, src.data_ptr(), src.numel(), n, src_off.data_ptr(),
                                                       record.data_ptr() if record is not None else None))

    def train_dict_async(self, src: torch.Tensor, src_off: torch.Tensor, dict_out: torch.Tensor, params: "TrainParams | None" = None,
                         record: "torch.Tensor | None" = None):
        """Enqueue the training of a dictionary from a batch of samples: sample i is src[src_off[i]:src_off[i+1]] (src: a uint8 device
        tensor; src_off: an int64 device tensor of n+1 offsets; overlapping spans are legal, a span that runs backwards or past src
        gives nothing), and dict_out (a uint8 device tensor of at most 65 536 bytes) receives the dictionary - all of it is written:
        the trained content right-aligned, the best segments last, zeros in front - so that create_cdict(dict_out) follows on the
        same stream with no size read back.  The segments are those of the samples whose params.d-byte substrings are the most
        frequent in the batch, params.k bytes each at most, chosen in up to params.rounds rounds (TrainParams; None and every field
        left 0: the defaults, TRAIN_DEFAULTS); the bytes are those of the sequential definition in include/lz4f_mi355x.h, whatever
        the device does in parallel.
        record (uint8 device tensor of 32 bytes, optional) receives one Result: size = the trained bytes, consumed = the sample
        bytes taken, n_blocks = the segments, first_bad_block = the first sample whose span is invalid (0xFFFFFFFF: none), status 0,
        flags & 0xFF = the rounds run.  The call raises only for what is wrong with the call itself (DeviceCodecError for a
        parameter out of range).  Nothing is read back: no synchronisation.  On one stream:

            eng.train_dict_async(samples, samples_off, d)
            cd = eng.create_cdict(d)
            eng.compress_frames_async(inp, inp_off, win, win_off, prefs, results, cdict=cd)"""
        n = _check_train_args(src, src_off, dict_out, params, record, self.RESULT_BYTES)
        _chk(self.L, self.L.lz4f_mi355x_dev_trainDict(self.h, n, src.data_ptr(), src.numel(), src_off.data_ptr(), dict_out.data_ptr(), dict_out.numel(),
                                                     ctypes.byref(params) if params is not None else None,
                                                     record.data_ptr() if record is not None else None))

    def frame_results(self, results: torch.Tensor) -> "list[Result]":
        """Wait for the stream, then the records of a batch (status 0 = ok; otherwise the LZ4F error code of that frame)."""
        self.stream.synchronize()
        raw = results.cpu().numpy().tobytes()
        return [Result.from_buffer_copy(raw, k) for k in range(0, len(raw) - self.RESULT_BYTES + 1, self.RESULT_BYTES)]

    def result(self) -> Result:
        r = self._result()                                   # (waits for the stream: everything enqueued so far, then the record's copy)
        if r.status != 0:
            raise DeviceCodecError("%s at block %d" % (self.L.LZ4F_getErrorName((1 << 64) - r.status).decode(), r.first_bad_block))
        return r

    def new_table(self, n_blocks: int) -> torch.Tensor:
        return torch.zeros((n_blocks + 1) * ctypes.sizeof(Block), dtype=torch.uint8, device="cuda:%d" % self.device)

    def index_size(self, n: int, prefs: Preferences) -> int:
        return int(self.L.lz4f_mi355x_dev_index_size(n, ctypes.byref(prefs)))

    def new_index(self, n: int, prefs: Preferences) -> torch.Tensor:
        return torch.zeros(self.index_size(n, prefs), dtype=torch.uint8, device="cuda:%d" % self.device)

    def xxh32(self, base: torch.Tensor, offs: np.ndarray, lens: np.ndarray) -> np.ndarray:
        dev = "cuda:%d" % self.device
        o = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64)).to(dev)
        l = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint32).view(np.int32)).to(dev)
        out = torch.zeros(len(lens), dtype=torch.int32, device=dev)
        _chk(self.L, self.L.lz4f_mi355x_dev_xxh32(self.h, base.data_ptr(), o.data_ptr(), l.data_ptr(), len(lens), out.data_ptr()))
        self.stream.synchronize()
        return out.cpu().numpy().view(np.uint32)


def synth50_device(n: int, seed: int, device: str = "cuda:0") -> torch.Tensor:
    """synth50 recipe (datagen.synth50) generated in HBM with torch's generator: 512-byte rows, even rows
    random, odd row r = copy of even row r-(2k+1), k in [1,60).  Same structure as the numpy version,
    different RNG stream (the numpy one is the canonical input of the parity tests)."""
    assert n % 1024 == 0
    g = torch.Generator(device=device); g.manual_seed(seed)
    rows = n // 512
    a = torch.randint(0, 256, (rows, 512), dtype=torch.uint8, device=device, generator=g)
    odd = torch.arange(1, rows, 2, device=device)
    back = torch.randint(1, 60, (odd.numel(),), device=device, generator=g) * 2 + 1
    src = torch.clamp(odd - back, min=0)
    src = src - (src % 2)
    a[odd] = a[src]
    return a.reshape(-1)
