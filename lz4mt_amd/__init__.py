"""lz4mt_amd — MI355X-native LZ4 frame codec behind the t-mat/lz4mt API.

The product is the C-ABI library ``liblz4mt_amd.so`` (HIP kernels for gfx950
+ the C++ frame engine).  This package is the Python host mirror of the
reference's interface (src/lz4mt.h): ``init_context``,
``init_stream_descriptor``, ``compress`` / ``decompress`` over callbacks,
plus device-resident helpers that take torch tensors (torch supplies device
memory and streams only).

torch is imported before the library is loaded so that both bind the same
libamdhip64 (identical soname); there is no CPU fallback: on a machine
without a HIP device every compute entry point returns an error.
"""
import ctypes
import weakref

import torch  # noqa: F401  (must precede the CDLL load: shared HIP runtime)

from . import _abi
from ._abi import (MODE_DEVICE, MODE_PARALLEL, MODE_SEQUENTIAL, RESULT_NAMES, Lz4MtContext, Lz4MtMemIo,
                   Lz4MtStreamDescriptor, Result)

__all__ = [
    "lib", "Result", "RESULT_NAMES", "MODE_PARALLEL", "MODE_SEQUENTIAL", "MODE_DEVICE", "Lz4MtError",
    "init_context", "init_stream_descriptor", "result_to_string", "result_to_exit_code", "make_sd",
    "compress", "decompress", "compress_block", "decompress_block", "compress_bound",
    "compress_frame", "decompress_frame", "frame_info", "frame_bound", "gen_synthetic", "xxh32",
    "device_count", "stream_bound", "frame_records", "xxh32_chunks", "frame_header", "shard_workspace",
    "shard_pack_bound", "shard_reset", "shard_encode", "shard_pack", "shard_unpack", "shard_assemble", "shard_body_bytes",
    "batch_compress_bound", "compress_batch", "decompress_batch", "BATCH_MAX_CHUNK", "BATCH_BAD_CHUNK",
    "batch_compress_workspace", "BATCH_HC_SLOTS",
    "DICT_WINDOW", "PreparedDict", "prepare_dict", "compress_batch_dict", "decompress_batch_dict",
    "prepare_dict_hc", "compress_batch_dict_hc", "batch_compress_dict_workspace",
    "BATCH_NO_DICT", "PreparedDictSet", "prepare_dict_set", "compress_batch_dict_set", "decompress_batch_dict_set",
    "prepare_dict_set_hc", "compress_batch_dict_set_hc",
]

lib = _abi.load()


class Lz4MtError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = int(code)
        name = RESULT_NAMES[code] if 0 <= code < len(RESULT_NAMES) else result_to_string(code)
        super().__init__(f"{what}: {name} ({code})")


def init_context():
    """lz4mtInitContext (reference src/lz4mt.cpp:851-871)."""
    return lib.lz4mtInitContext()


def init_stream_descriptor():
    """lz4mtInitStreamDescriptor (reference src/lz4mt.cpp:874-895)."""
    return lib.lz4mtInitStreamDescriptor()


def result_to_string(code):
    return lib.lz4mtResultToString(int(code)).decode()


def result_to_exit_code(code):
    return lib.lz4mtResultToLz4cExitCode(int(code))


def make_sd(block_max_id=7, stream_checksum=True, block_checksum=False, stream_size=None, block_dependence=False):
    """Stream descriptor with the CLI's flag mapping (-B#, -BX, -BD, -Sx)."""
    sd = init_stream_descriptor()
    sd.bd.blockMaximumSize = block_max_id
    sd.flg.blockIndependence = 0 if block_dependence else 1
    sd.flg.streamChecksum = 1 if stream_checksum else 0
    sd.flg.blockChecksum = 1 if block_checksum else 0
    if stream_size is not None:
        sd.flg.streamSize = 1
        sd.streamSize = int(stream_size)
    return sd


def device_count():
    return lib.lz4mtHipDeviceCount()


# ---------------------------------------------------------------------------
# callback API over memory buffers (lz4mtCompress / lz4mtDecompress)
# ---------------------------------------------------------------------------
def _run(fn, data, sd, mode, level, out_cap, compress_cb=None, decompress_cb=None):
    src = ctypes.create_string_buffer(bytes(data), len(data) or 1)
    out = ctypes.create_string_buffer(max(out_cap, 1))
    io = Lz4MtMemIo(ctypes.cast(src, ctypes.c_void_p), len(data), 0, 0, ctypes.cast(out, ctypes.c_void_p),
                    out_cap, 0)
    ctx = init_context()
    ctx.mode = mode
    ctx.compressionLevel = level
    lib.lz4mtMemBind(ctypes.byref(ctx), ctypes.byref(io))
    keep = []
    if compress_cb is not None:
        keep.append(_abi.COMPRESS_FN(compress_cb))
        ctx.compress = ctypes.cast(keep[-1], ctypes.c_void_p)
    if decompress_cb is not None:
        keep.append(_abi.DECOMPRESS_FN(decompress_cb))
        ctx.decompress = ctypes.cast(keep[-1], ctypes.c_void_p)
    r = fn(ctypes.byref(ctx), ctypes.byref(sd))
    return r, out.raw[:io.outPos]


def compress(data, sd=None, mode=MODE_PARALLEL, level=0, compress_cb=None):
    """Frame-compresses ``data`` through lz4mtCompress; returns (result, frame bytes).

    Null codec callbacks run every block on the GPU (lz4mtHipCompressBlock);
    ``mode=MODE_DEVICE`` uses the batched device engine.
    """
    sd = sd if sd is not None else init_stream_descriptor()
    bm = 1 << (8 + 2 * sd.bd.blockMaximumSize) if 4 <= sd.bd.blockMaximumSize <= 7 else 4 << 20
    cap = 64 + len(data) + 8 * (len(data) // bm + 2)
    return _run(lib.lz4mtCompress, data, sd, mode, level, cap, compress_cb=compress_cb)


def decompress(frame, out_cap, mode=MODE_PARALLEL, decompress_cb=None):
    """lz4mtDecompress over memory; returns (result, decoded bytes, last stream descriptor)."""
    sd = init_stream_descriptor()
    r, out = _run(lib.lz4mtDecompress, frame, sd, mode, 0, out_cap, decompress_cb=decompress_cb)
    return r, out, sd


# ---------------------------------------------------------------------------
# block operators (reference plugin signatures, host memory)
# ---------------------------------------------------------------------------
def compress_bound(n):
    return lib.lz4mtHipCompressBound(int(n))


def compress_block(data, cap=None, level=0):
    """lz4mtHipCompressBlock: LZ4_compress_limitedOutput semantics; returns bytes (b'' if it does not fit)."""
    data = bytes(data)
    cap = len(data) if cap is None else int(cap)
    dst = ctypes.create_string_buffer(max(cap, compress_bound(len(data))) + 16)
    n = lib.lz4mtHipCompressBlock(data, dst, len(data), cap, level)
    if n < 0:
        raise Lz4MtError(Result.ERROR, "lz4mtHipCompressBlock")
    return dst.raw[:n]


def decompress_block(block, cap):
    """lz4mtHipDecompressBlock: returns (ret, bytes) with ret < 0 for malformed input."""
    block = bytes(block)
    dst = ctypes.create_string_buffer(max(int(cap), 1) + 16)
    n = lib.lz4mtHipDecompressBlock(block, dst, len(block), int(cap))
    return n, (dst.raw[:n] if n > 0 else b"")


# ---------------------------------------------------------------------------
# device-resident frame engine (torch uint8 tensors on the current device)
# ---------------------------------------------------------------------------
def _stream(stream):
    if stream is None:
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return ctypes.c_void_p(stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))


def _check_dev(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous torch.uint8 tensor on a HIP device")


# ---------------------------------------------------------------------------
# batched block operators on device memory (include/lz4mt_hip.h section 5)
# ---------------------------------------------------------------------------
BATCH_MAX_CHUNK = _abi.BATCH_MAX_CHUNK
BATCH_BAD_CHUNK = _abi.BATCH_BAD_CHUNK
BATCH_HC_SLOTS = _abi.BATCH_HC_SLOTS


def batch_compress_bound(n):
    """Capacity at which a chunk of ``n`` bytes always fits (lz4mtHipCompressBound)."""
    return compress_bound(n)


def batch_compress_workspace(max_chunk, n, level, device=None):
    """Scratch for compress_batch / lz4mtHipCompressBatchEx at ``level`` over
    ``n`` chunks of at most ``max_chunk`` bytes: a uint8 tensor of
    lz4mtHipCompressBatchWorkspaceSize bytes (empty below level 3).  The call
    accepts any workspace of at least one slot (``n = 1``) and runs more rounds
    with fewer slots."""
    nbytes = int(lib.lz4mtHipCompressBatchWorkspaceSize(int(max_chunk), int(n), int(level)))
    return torch.empty(nbytes, dtype=torch.uint8, device=device or "cuda")


def _batch(fn_name, srcs, caps, null_caps, max_chunk, stream, level=0, workspace=None, dict_args=None):
    """The common part of compress_batch / decompress_batch: one backing
    allocation for the outputs (each at a 16-byte-aligned offset, ``cap``
    bytes long), the four descriptor arrays built on the host and uploaded
    in one copy, one library call.  Everything is issued on ``stream``.
    ``level`` >= 3 (compress only): lz4mtHipCompressBatchEx, its workspace
    allocated here on the call's stream unless one is given.
    ``dict_args`` (the dictionary calls): the arguments between d_outSizes
    and the stream (with ``level`` >= 3: and the level), as ctypes values;
    at ``level`` >= 3 they go to the LZ4-HC call of ``fn_name``'s section."""
    n = len(srcs)
    dev = srcs[0].device if n else torch.device("cuda", torch.cuda.current_device())
    if stream is None:
        ts = torch.cuda.current_stream(dev)
    elif isinstance(stream, torch.cuda.Stream):
        ts = stream
    else:
        ts = torch.cuda.ExternalStream(int(stream), device=dev)
    with torch.cuda.stream(ts):
        sizes = torch.empty(n, dtype=torch.int32, device=dev)
        if n == 0:
            return [], sizes
        offs, total = [], 0
        for c in caps:
            offs.append(total)
            total += (c + 15) & ~15
        back = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        base = back.data_ptr()
        assert base % 16 == 0
        # [src pointers | dst pointers] as int64, then [src sizes | capacities] as int32, in one host buffer
        # (pinned, so that the upload is asynchronous too: the host allocator
        # keeps the buffer until the copy has run)
        host = torch.empty(2 * n * 8 + 2 * n * 4, dtype=torch.uint8, pin_memory=True)
        p64 = host[:16 * n].view(torch.int64)
        p64[:n] = torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64)
        p64[n:] = torch.tensor([base + o for o in offs], dtype=torch.int64)
        p32 = host[16 * n:].view(torch.int32)
        p32[:n] = torch.tensor([s.numel() for s in srcs], dtype=torch.int64).to(torch.int32)   # (u32 bit patterns)
        p32[n:] = torch.tensor(caps, dtype=torch.int64).to(torch.int32)
        desc = host.to(dev, non_blocking=True)
        d = desc.data_ptr()
        d_src, d_dst, d_sz, d_cap = d, d + 8 * n, d + 16 * n, d + 20 * n
        fn = getattr(lib, fn_name)
        st = ctypes.c_void_p(ts.cuda_stream)
        cap_arg = ctypes.c_void_p(None if null_caps else d_cap)
        if level >= 3:
            if dict_args is not None:   # (dictionary, size, HC state): section 5c; the set's arrays: section 5e
                if workspace is None:
                    workspace = batch_compress_dict_workspace(max_chunk, n, level, device=dev)
                fn_name = "lz4mtHipCompressBatchDictSetHC" if fn_name == "lz4mtHipCompressBatchDictSet" else \
                    "lz4mtHipCompressBatchDictHC"
                r = getattr(lib, fn_name)(ctypes.c_void_p(d_src), ctypes.c_void_p(d_sz), max_chunk, n,
                                          ctypes.c_void_p(d_dst), cap_arg, ctypes.c_void_p(sizes.data_ptr()),
                                          *dict_args, level, ctypes.c_void_p(workspace.data_ptr()),
                                          workspace.numel(), st)
                if r != Result.OK:
                    raise Lz4MtError(r, fn_name)
                return [back[o:o + c] for o, c in zip(offs, caps)], sizes
            if workspace is None:
                workspace = batch_compress_workspace(max_chunk, n, level, device=dev)
            fn_name = "lz4mtHipCompressBatchEx"
            r = lib.lz4mtHipCompressBatchEx(ctypes.c_void_p(d_src), ctypes.c_void_p(d_sz), max_chunk, n,
                                            ctypes.c_void_p(d_dst), cap_arg, ctypes.c_void_p(sizes.data_ptr()),
                                            level, ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), st)
        elif max_chunk is None:
            r = fn(ctypes.c_void_p(d_src), ctypes.c_void_p(d_sz), n, ctypes.c_void_p(d_dst), cap_arg,
                   ctypes.c_void_p(sizes.data_ptr()), *(dict_args or ()), st)
        else:
            r = fn(ctypes.c_void_p(d_src), ctypes.c_void_p(d_sz), max_chunk, n, ctypes.c_void_p(d_dst), cap_arg,
                   ctypes.c_void_p(sizes.data_ptr()), *(dict_args or ()), st)
        if r != Result.OK:
            raise Lz4MtError(r, fn_name)
        return [back[o:o + c] for o, c in zip(offs, caps)], sizes


def compress_batch(chunks, caps=None, stream=None, level=0, workspace=None):
    """lz4mtHipCompressBatch: every tensor of ``chunks`` (contiguous uint8 on
    one HIP device, slices at any offset included, at most 4 MiB each) as an
    independent raw LZ4 block, in one launch.  ``caps``: a capacity per chunk
    (default: the bound of each size).  Returns ``(outs, sizes)``: ``outs[i]``
    a ``caps[i]``-byte view of one backing allocation, ``sizes`` the int32
    device tensor of block sizes (0: does not fit its capacity).  Does not
    synchronise: ``chunks`` must stay alive until ``stream`` has run the call.
    ``level`` >= 3: LZ4-HC through lz4mtHipCompressBatchEx (one wave per chunk
    and a launch pair per round); ``workspace``: a uint8 device tensor of at
    least one slot (batch_compress_workspace), kept alive and untouched until
    the call has run -- by default one of the full size is allocated on the
    call's stream."""
    chunks = list(chunks)
    level = int(level)
    if workspace is not None and level >= 3:
        _check_dev(workspace, "workspace")
    for i, c in enumerate(chunks):
        _check_dev(c, f"chunks[{i}]")
    big = max((c.numel() for c in chunks), default=0)
    if big > BATCH_MAX_CHUNK:
        raise ValueError(f"a chunk of {big} bytes exceeds the batch maximum of {BATCH_MAX_CHUNK}")
    if caps is None:
        return _batch("lz4mtHipCompressBatch", chunks, [batch_compress_bound(c.numel()) for c in chunks], True, big,
                      stream, level, workspace)
    caps = [int(c) for c in caps]
    if len(caps) != len(chunks) or any(c < 0 or c >= 1 << 32 for c in caps):
        raise ValueError("caps: one capacity of 0 .. 2^32 - 1 per chunk")
    return _batch("lz4mtHipCompressBatch", chunks, caps, False, big, stream, level, workspace)


def decompress_batch(blocks, caps, stream=None):
    """lz4mtHipDecompressBatch: every tensor of ``blocks`` (contiguous uint8
    on one HIP device) is one raw LZ4 block, decoded into at most ``caps[i]``
    bytes, in one launch.  Returns ``(outs, sizes)`` as
    compress_batch does; ``sizes[i]`` is the decoded size, negative for a
    malformed block (LZ4_decompress_safe).  Does not synchronise."""
    blocks = list(blocks)
    for i, b in enumerate(blocks):
        _check_dev(b, f"blocks[{i}]")
    caps = [int(c) for c in caps]
    if len(caps) != len(blocks) or any(c < 0 or c >= 1 << 31 for c in caps):
        raise ValueError("caps: one capacity of 0 .. 2^31 - 1 per block")
    return _batch("lz4mtHipDecompressBatch", blocks, caps, False, None, stream)


# the same with a dictionary shared by every chunk (lz4mt_hip.h section 5b)
DICT_WINDOW = _abi.DICT_WINDOW


class PreparedDict:
    """A dictionary ready for compress_batch_dict: ``dictionary`` (the
    caller's uint8 device tensor, kept alive here) and ``state`` (the
    lz4mtHipDictPrepare state, a uint8 device tensor of
    lz4mtHipDictStateSize bytes).  ``kind``: "fast" (lz4mtHipDictPrepare, for
    compress_batch_dict) or "hc" (lz4mtHipDictPrepareHC, a state of
    lz4mtHipDictStateSizeHC bytes, for compress_batch_dict_hc); ``is_hc``
    tells them apart."""
    __slots__ = ("dictionary", "state", "kind")

    def __init__(self, dictionary, state, kind="fast"):
        self.dictionary = dictionary
        self.state = state
        self.kind = kind

    @property
    def is_hc(self):
        return self.kind == "hc"


def _dict_ptr(dictionary):
    return ctypes.c_void_p(dictionary.data_ptr() if dictionary.numel() else None), dictionary.numel()


def batch_compress_dict_workspace(max_chunk, n, level, device=None):
    """Scratch for compress_batch_dict_hc at ``level``
    (lz4mtHipCompressBatchDictWorkspaceSize bytes; empty below level 3): the
    slots and rounds of batch_compress_workspace."""
    nbytes = int(lib.lz4mtHipCompressBatchDictWorkspaceSize(int(max_chunk), int(n), int(level)))
    return torch.empty(nbytes, dtype=torch.uint8, device=device or "cuda")


def prepare_dict(dictionary, stream=None):
    """lz4mtHipDictPrepare: builds, with one kernel on ``stream``, the table
    LZ4_loadDict leaves for ``dictionary`` (a contiguous uint8 device tensor
    of any size and alignment; its last 64 KiB count, fewer than 8 bytes are
    no dictionary).  Returns a PreparedDict.  Does not synchronise."""
    return _prepare_dict(dictionary, stream, False)


def prepare_dict_hc(dictionary, stream=None):
    """lz4mtHipDictPrepareHC: the same for compress_batch_dict_hc -- what
    LZ4_loadDictHC leaves (the last 64 KiB count, whatever their number).  The
    one state serves every level from 3 up.  Returns a PreparedDict of kind
    "hc".  Does not synchronise."""
    return _prepare_dict(dictionary, stream, True)


def _prepare_dict(dictionary, stream, hc):
    size_fn, prep_fn = (lib.lz4mtHipDictStateSizeHC, lib.lz4mtHipDictPrepareHC) if hc else \
        (lib.lz4mtHipDictStateSize, lib.lz4mtHipDictPrepare)
    _check_dev(dictionary, "dictionary")
    if dictionary.numel() >= 1 << 32:
        raise ValueError("a dictionary is at most 2^32 - 1 bytes")
    dev = dictionary.device
    if stream is None:
        ts = torch.cuda.current_stream(dev)
    elif isinstance(stream, torch.cuda.Stream):
        ts = stream
    else:
        ts = torch.cuda.ExternalStream(int(stream), device=dev)
    with torch.cuda.stream(ts):
        state = torch.empty(int(size_fn()), dtype=torch.uint8, device=dev)
        dptr, dsize = _dict_ptr(dictionary)
        r = prep_fn(dptr, dsize, ctypes.c_void_p(state.data_ptr()), state.numel(), ctypes.c_void_p(ts.cuda_stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipDictPrepareHC" if hc else "lz4mtHipDictPrepare")
    return PreparedDict(dictionary, state, "hc" if hc else "fast")


def compress_batch_dict(chunks, prepared, caps=None, stream=None):
    """lz4mtHipCompressBatchDict: compress_batch (the fast codec) with the
    dictionary of ``prepared`` (prepare_dict) before every chunk: the bytes of
    LZ4_loadDict + LZ4_compress_fast_continue.  Returns ``(outs, sizes)`` as
    compress_batch does; decode with decompress_batch_dict and the same
    dictionary.  Does not synchronise: ``chunks`` and ``prepared`` must stay
    alive until ``stream`` has run the call, and ``stream`` must be ordered
    after the one prepare_dict ran on.  A PreparedDict of kind "hc"
    (prepare_dict_hc) is a TypeError: LZ4-HC is compress_batch_dict_hc."""
    return _compress_batch_dict(chunks, prepared, caps, stream, 0, None)


def compress_batch_dict_hc(chunks, prepared, level, caps=None, stream=None, workspace=None):
    """lz4mtHipCompressBatchDictHC: compress_batch at ``level`` 3..12 (LZ4-HC)
    with the dictionary of ``prepared`` (prepare_dict_hc; a PreparedDict of
    kind "fast" is a TypeError) before every chunk: the bytes of
    LZ4_loadDictHC + LZ4_compress_HC_continue.  Everything else as
    compress_batch_dict; ``workspace`` as for compress_batch
    (batch_compress_dict_workspace; by default one of the full size is
    allocated on the call's stream)."""
    level = int(level)
    if level < 3:
        raise ValueError("compress_batch_dict_hc: level 3..12 (the fast codec is compress_batch_dict)")
    return _compress_batch_dict(chunks, prepared, caps, stream, level, workspace)


def _compress_batch_dict(chunks, prepared, caps, stream, level, workspace):
    if not isinstance(prepared, PreparedDict):
        raise TypeError("prepared must come from prepare_dict / prepare_dict_hc")
    if prepared.is_hc != (level >= 3):
        raise TypeError("compress_batch_dict takes a prepare_dict state, compress_batch_dict_hc a prepare_dict_hc state")
    if workspace is not None:
        _check_dev(workspace, "workspace")
    chunks = list(chunks)
    for i, c in enumerate(chunks):
        _check_dev(c, f"chunks[{i}]")
    big = max((c.numel() for c in chunks), default=0)
    if big > BATCH_MAX_CHUNK:
        raise ValueError(f"a chunk of {big} bytes exceeds the batch maximum of {BATCH_MAX_CHUNK}")
    dptr, dsize = _dict_ptr(prepared.dictionary)
    dict_args = (dptr, dsize, ctypes.c_void_p(prepared.state.data_ptr()))
    if caps is None:
        return _batch("lz4mtHipCompressBatchDict", chunks, [batch_compress_bound(c.numel()) for c in chunks], True,
                      big, stream, level, workspace, dict_args=dict_args)
    caps = [int(c) for c in caps]
    if len(caps) != len(chunks) or any(c < 0 or c >= 1 << 32 for c in caps):
        raise ValueError("caps: one capacity of 0 .. 2^32 - 1 per chunk")
    return _batch("lz4mtHipCompressBatchDict", chunks, caps, False, big, stream, level, workspace, dict_args=dict_args)


def decompress_batch_dict(blocks, caps, dictionary, stream=None):
    """lz4mtHipDecompressBatchDict: decompress_batch against ``dictionary``
    (a uint8 device tensor, or the PreparedDict the blocks were compressed
    with): LZ4_decompress_safe_usingDict per block.  Does not synchronise."""
    if isinstance(dictionary, PreparedDict):
        dictionary = dictionary.dictionary
    _check_dev(dictionary, "dictionary")
    blocks = list(blocks)
    for i, b in enumerate(blocks):
        _check_dev(b, f"blocks[{i}]")
    caps = [int(c) for c in caps]
    if len(caps) != len(blocks) or any(c < 0 or c >= 1 << 31 for c in caps):
        raise ValueError("caps: one capacity of 0 .. 2^31 - 1 per block")
    return _batch("lz4mtHipDecompressBatchDict", blocks, caps, False, None, stream, dict_args=_dict_ptr(dictionary))


# a set of dictionaries and an index per chunk (lz4mt_hip.h section 5d)
BATCH_NO_DICT = _abi.BATCH_NO_DICT


class PreparedDictSet:
    """A set of dictionaries ready for compress_batch_dict_set:
    ``dictionaries`` (the caller's uint8 device tensors, kept alive here),
    ``ptrs`` (int64) and ``sizes`` (int32, u32 bit patterns): the device
    arrays lz4mtHipDictSetPrepare read, and ``states``: a uint8 device tensor
    of ``len(dictionaries)`` states of lz4mtHipDictStateSize bytes each, or
    None when the set was built for decoding only.  ``kind``: "fast"
    (prepare_dict_set, for compress_batch_dict_set) or "hc"
    (prepare_dict_set_hc: states of lz4mtHipDictStateSizeHC bytes, for
    compress_batch_dict_set_hc); ``is_hc`` tells them apart."""
    __slots__ = ("dictionaries", "ptrs", "sizes", "states", "kind")

    def __init__(self, dictionaries, ptrs, sizes, states, kind="fast"):
        self.dictionaries = dictionaries
        self.ptrs = ptrs
        self.sizes = sizes
        self.states = states
        self.kind = kind

    @property
    def is_hc(self):
        return self.kind == "hc"

    def __len__(self):
        return len(self.dictionaries)


def _torch_stream(stream, dev):
    if stream is None:
        return torch.cuda.current_stream(dev)
    if isinstance(stream, torch.cuda.Stream):
        return stream
    return torch.cuda.ExternalStream(int(stream), device=dev)


def _dict_set(dictionaries, stream, states, hc=False):
    """The device arrays of a set (uploaded on ``stream`` from pinned memory,
    no synchronisation) and, with ``states``, lz4mtHipDictSetPrepare (``hc``:
    lz4mtHipDictSetPrepareHC)."""
    dictionaries = list(dictionaries)
    for i, d in enumerate(dictionaries):
        _check_dev(d, f"dictionaries[{i}]")
        if d.numel() >= 1 << 32:
            raise ValueError("a dictionary is at most 2^32 - 1 bytes")
    k = len(dictionaries)
    dev = dictionaries[0].device if k else torch.device("cuda", torch.cuda.current_device())
    ts = _torch_stream(stream, dev)
    with torch.cuda.stream(ts):
        host = torch.empty(max(12 * k, 16), dtype=torch.uint8, pin_memory=True)   # [pointers | sizes]
        host[:8 * k].view(torch.int64)[:] = torch.tensor([d.data_ptr() if d.numel() else 0 for d in dictionaries],
                                                         dtype=torch.int64)
        host[8 * k:12 * k].view(torch.int32)[:] = torch.tensor([d.numel() for d in dictionaries],
                                                               dtype=torch.int64).to(torch.int32)
        desc = host.to(dev, non_blocking=True)
        ptrs, sizes = desc[:8 * k].view(torch.int64), desc[8 * k:12 * k].view(torch.int32)
        st = None
        if states:
            size_fn, prep = (lib.lz4mtHipDictStateSizeHC, "lz4mtHipDictSetPrepareHC") if hc else \
                (lib.lz4mtHipDictStateSize, "lz4mtHipDictSetPrepare")
            st = torch.empty(k * int(size_fn()), dtype=torch.uint8, device=dev)
            assert st.data_ptr() % 256 == 0
            r = getattr(lib, prep)(ctypes.c_void_p(ptrs.data_ptr()), ctypes.c_void_p(sizes.data_ptr()), k,
                                   ctypes.c_void_p(st.data_ptr()), st.numel(), ctypes.c_void_p(ts.cuda_stream))
            if r != Result.OK:
                raise Lz4MtError(r, prep)
    return PreparedDictSet(dictionaries, ptrs, sizes, st, "hc" if hc else "fast")


def prepare_dict_set(dictionaries, stream=None):
    """lz4mtHipDictSetPrepare: what prepare_dict does, for every tensor of
    ``dictionaries`` (contiguous uint8 on one HIP device, any size and
    alignment) with one kernel on ``stream``.  Returns a PreparedDictSet.
    Does not synchronise."""
    return _dict_set(dictionaries, stream, True)


def prepare_dict_set_hc(dictionaries, stream=None):
    """lz4mtHipDictSetPrepareHC: what prepare_dict_hc does, for every tensor of
    ``dictionaries``, one workgroup per dictionary on ``stream``.  The states
    serve every level from 3 up.  Returns a PreparedDictSet of kind "hc" (for
    compress_batch_dict_set_hc and decompress_batch_dict_set).  Does not
    synchronise."""
    return _dict_set(dictionaries, stream, True, hc=True)


def _which(which, n, k, dev, ts):
    """``which`` (an int below ``k`` or None per chunk) as the device array
    d_chunkDict, uploaded on ``ts``."""
    which = list(which)
    if len(which) != n:
        raise ValueError("which: one entry per chunk")
    idx = []
    for w in which:
        if w is None:
            idx.append(BATCH_NO_DICT)
        elif 0 <= int(w) < k:
            idx.append(int(w))
        else:
            raise ValueError(f"which: {w!r} names none of the {k} dictionaries")
    with torch.cuda.stream(ts):
        host = torch.empty(max(n, 1), dtype=torch.int32, pin_memory=True)
        host[:n] = torch.tensor(idx, dtype=torch.int64).to(torch.int32)   # (u32 bit patterns)
        return host.to(dev, non_blocking=True)


def compress_batch_dict_set(chunks, prepared, which, caps=None, stream=None):
    """lz4mtHipCompressBatchDictSet: compress_batch_dict with a dictionary per
    chunk, in one launch: chunk ``i`` gets dictionary ``which[i]`` of
    ``prepared`` (prepare_dict_set), or none when ``which[i]`` is None.
    Returns ``(outs, sizes)`` as compress_batch does; decode with
    decompress_batch_dict_set, the same set and the same ``which``.  Does not
    synchronise: ``chunks`` and ``prepared`` must stay alive until ``stream``
    has run the call, and ``stream`` must be ordered after the one
    prepare_dict_set ran on.  A PreparedDictSet of kind "hc"
    (prepare_dict_set_hc) is a TypeError: LZ4-HC is compress_batch_dict_set_hc."""
    return _compress_batch_dict_set(chunks, prepared, which, caps, stream, 0, None)


def compress_batch_dict_set_hc(chunks, prepared, which, level, caps=None, stream=None, workspace=None):
    """lz4mtHipCompressBatchDictSetHC: compress_batch_dict_hc at ``level``
    3..12 with a dictionary per chunk, in one call: chunk ``i`` gets
    dictionary ``which[i]`` of ``prepared`` (prepare_dict_set_hc; a set of kind
    "fast" is a TypeError), or compress_batch's bytes at ``level`` when
    ``which[i]`` is None.  Everything else as compress_batch_dict_set;
    ``workspace`` as for compress_batch_dict_hc."""
    level = int(level)
    if level < 3:
        raise ValueError("compress_batch_dict_set_hc: level 3..12 (the fast codec is compress_batch_dict_set)")
    return _compress_batch_dict_set(chunks, prepared, which, caps, stream, level, workspace)


def _compress_batch_dict_set(chunks, prepared, which, caps, stream, level, workspace):
    if not isinstance(prepared, PreparedDictSet) or prepared.states is None:
        raise TypeError("prepared must come from prepare_dict_set / prepare_dict_set_hc")
    if prepared.is_hc != (level >= 3):
        raise TypeError("compress_batch_dict_set takes a prepare_dict_set set, "
                        "compress_batch_dict_set_hc a prepare_dict_set_hc set")
    if workspace is not None:
        _check_dev(workspace, "workspace")
    chunks = list(chunks)
    for i, c in enumerate(chunks):
        _check_dev(c, f"chunks[{i}]")
    big = max((c.numel() for c in chunks), default=0)
    if big > BATCH_MAX_CHUNK:
        raise ValueError(f"a chunk of {big} bytes exceeds the batch maximum of {BATCH_MAX_CHUNK}")
    null_caps = caps is None
    if null_caps:
        caps = [batch_compress_bound(c.numel()) for c in chunks]
    else:
        caps = [int(c) for c in caps]
        if len(caps) != len(chunks) or any(c < 0 or c >= 1 << 32 for c in caps):
            raise ValueError("caps: one capacity of 0 .. 2^32 - 1 per chunk")
    dev = chunks[0].device if chunks else prepared.states.device
    ts = _torch_stream(stream, dev)
    idx = _which(which, len(chunks), len(prepared), dev, ts)
    dict_args = (ctypes.c_void_p(prepared.ptrs.data_ptr()), ctypes.c_void_p(prepared.sizes.data_ptr()),
                 len(prepared), ctypes.c_void_p(prepared.states.data_ptr()), ctypes.c_void_p(idx.data_ptr()))
    return _batch("lz4mtHipCompressBatchDictSet", chunks, caps, null_caps, big, ts, level, workspace,
                  dict_args=dict_args)


def decompress_batch_dict_set(blocks, caps, dictionaries, which, stream=None):
    """lz4mtHipDecompressBatchDictSet: decompress_batch_dict with a dictionary
    per block, in one launch.  ``dictionaries``: the PreparedDictSet the
    blocks were compressed with (of either kind: only its dictionaries are
    used), or a list of uint8 device tensors;
    ``which[i]``: the index of block ``i``'s dictionary, or None for a block
    made without one.  Does not synchronise."""
    blocks = list(blocks)
    for i, b in enumerate(blocks):
        _check_dev(b, f"blocks[{i}]")
    caps = [int(c) for c in caps]
    if len(caps) != len(blocks) or any(c < 0 or c >= 1 << 31 for c in caps):
        raise ValueError("caps: one capacity of 0 .. 2^31 - 1 per block")
    if not isinstance(dictionaries, PreparedDictSet):
        dictionaries = _dict_set(dictionaries, stream, False)
    dev = blocks[0].device if blocks else dictionaries.ptrs.device
    ts = _torch_stream(stream, dev)
    idx = _which(which, len(blocks), len(dictionaries), dev, ts)
    dict_args = (ctypes.c_void_p(dictionaries.ptrs.data_ptr()), ctypes.c_void_p(dictionaries.sizes.data_ptr()),
                 len(dictionaries), ctypes.c_void_p(idx.data_ptr()))
    return _batch("lz4mtHipDecompressBatchDictSet", blocks, caps, False, None, ts, dict_args=dict_args)


def frame_bound(n, sd=None):
    sd = sd if sd is not None else init_stream_descriptor()
    return int(lib.lz4mtHipFrameBound(int(n), ctypes.byref(sd)))


def compress_workspace(n, sd=None, device=None, level=0):
    sd = sd if sd is not None else init_stream_descriptor()
    nbytes = int(lib.lz4mtHipCompressWorkspaceSizeEx(int(n), ctypes.byref(sd), int(level)))
    return torch.empty(nbytes, dtype=torch.uint8, device=device or "cuda")


def compress_frame(src, sd=None, out=None, workspace=None, stream=None, level=0):
    """Compresses a device tensor into one lz4mt frame; returns the frame tensor (a view of ``out``).
    ``level`` >= 3 selects LZ4-HC (the reference's codec for those levels:
    3..9 hashChain, 10..12 and above the optimal parser)."""
    _check_dev(src, "src")
    sd = sd if sd is not None else init_stream_descriptor()
    n = src.numel()
    cap = frame_bound(n, sd)
    if out is None:
        out = torch.empty(cap, dtype=torch.uint8, device=src.device)
    fs = ctypes.c_uint64(0)
    ws_ptr, ws_size = (workspace.data_ptr(), workspace.numel()) if workspace is not None else (None, 0)
    r = lib.lz4mtHipCompressFrameEx(ctypes.c_void_p(src.data_ptr() if n else out.data_ptr()), n,
                                    ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(fs),
                                    ctypes.byref(sd), int(level), ctypes.c_void_p(ws_ptr), ws_size, _stream(stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipCompressFrame")
    return out[:fs.value]


def frame_info(frame, stream=None):
    """(stream descriptor, decoded-size bound, block count) of the first frame."""
    _check_dev(frame, "frame")
    sd = init_stream_descriptor()
    bound, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    r = lib.lz4mtHipFrameInfo(ctypes.c_void_p(frame.data_ptr()), frame.numel(), ctypes.byref(sd),
                              ctypes.byref(bound), ctypes.byref(nb), _stream(stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipFrameInfo")
    return sd, bound.value, nb.value


def stream_bound(frame, stream=None):
    """Decoded-size bound of every frame in the device bytes (concatenated and skippable frames included)."""
    _check_dev(frame, "frame")
    b = ctypes.c_uint64(0)
    r = lib.lz4mtHipStreamBound(ctypes.c_void_p(frame.data_ptr()), frame.numel(), ctypes.byref(b), _stream(stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipStreamBound")
    return b.value


def frame_records(frame, frame_len=None, stream=None):
    """(header length, [record start offsets..., EOS offset], descriptor) of one device frame (device walk)."""
    _check_dev(frame, "frame")
    n = frame.numel() if frame_len is None else int(frame_len)
    sd = init_stream_descriptor()
    nb, hl = ctypes.c_uint64(0), ctypes.c_int(0)
    r = lib.lz4mtHipFrameRecords(ctypes.c_void_p(frame.data_ptr()), n, None, 0, ctypes.byref(nb), ctypes.byref(hl),
                                 ctypes.byref(sd), _stream(stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipFrameRecords")
    recs = (ctypes.c_uint64 * (nb.value + 1))()
    r = lib.lz4mtHipFrameRecords(ctypes.c_void_p(frame.data_ptr()), n, recs, nb.value + 1, ctypes.byref(nb),
                                 ctypes.byref(hl), ctypes.byref(sd), _stream(stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipFrameRecords")
    return hl.value, list(recs), sd


def xxh32_chunks(t, chunk=16 << 20, stream=None):
    """XXH32 of each consecutive ``chunk``-byte piece of a device tensor (int32 tensor of digests, same device)."""
    _check_dev(t, "tensor")
    nc = (t.numel() + chunk - 1) // chunk
    d = torch.empty(max(nc, 1), dtype=torch.int32, device=t.device)
    if nc and lib.lz4mtHipXxh32Chunks(ctypes.c_void_p(t.data_ptr()), t.numel(), chunk, ctypes.c_void_p(d.data_ptr()),
                                      _stream(stream)) != 0:
        raise Lz4MtError(Result.ERROR, "lz4mtHipXxh32Chunks")
    return d[:nc]


def decompress_frame(frame, out=None, stream=None, check=True):
    """Decompresses device frame bytes; returns (decoded tensor view, result code)."""
    _check_dev(frame, "frame")
    if out is None:
        out = torch.empty(max(stream_bound(frame, stream), 1), dtype=torch.uint8, device=frame.device)
    sd = init_stream_descriptor()
    osz = ctypes.c_uint64(0)
    r = lib.lz4mtHipDecompressFrame(ctypes.c_void_p(frame.data_ptr()), frame.numel(),
                                    ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.byref(osz),
                                    ctypes.byref(sd), _stream(stream))
    if check and r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipDecompressFrame")
    return out[:osz.value], r


def gen_synthetic(n, seed=42, device="cuda", stream=None):
    """SURVEY.md App. F synthetic input, generated on the device."""
    t = torch.empty(max(int(n), 1), dtype=torch.uint8, device=device)
    if lib.lz4mtHipGenSynthetic(ctypes.c_void_p(t.data_ptr()), int(n), int(seed), _stream(stream)) != 0:
        raise Lz4MtError(Result.ERROR, "lz4mtHipGenSynthetic")
    return t[:int(n)]


def xxh32(t, stream=None):
    """XXH32 (seed 0) of a device tensor, computed on the device."""
    _check_dev(t, "tensor")
    return int(lib.lz4mtHipXxh32(ctypes.c_void_p(t.data_ptr()), t.numel(), _stream(stream)))


# ---- block-sharded streamed gather (include/lz4mt_hip.h section 4; driven by dist.py)
PACK_HEADER_BYTES = 64


def frame_header(sd):
    """The frame header lz4mtCompress writes for ``sd`` (bytes)."""
    buf = (ctypes.c_uint8 * 20)()
    k = lib.lz4mtHipFrameHeader(ctypes.byref(sd), buf)
    if k < 0:
        raise Lz4MtError(Result.BAD_ARG, "lz4mtHipFrameHeader")
    return bytes(buf[:k])


def shard_workspace(n, sd, device=None):
    """Workspace of an n-byte shard encode (also the root's mirror of such a shard)."""
    nbytes = int(lib.lz4mtHipShardWorkspaceSize(int(n), ctypes.byref(sd)))
    if nbytes == 0:
        raise Lz4MtError(Result.BAD_ARG, "lz4mtHipShardWorkspaceSize (the descriptor does not shard)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device or "cuda")
    # the library keeps the Reset -> Encode -> Pack order per workspace
    # address: forget it when the tensor goes, so a later allocation at the
    # same address never inherits "encoded" 
    weakref.finalize(ws, lib.lz4mtHipShardRelease, ctypes.c_void_p(ws.data_ptr()))
    return ws


def shard_pack_bound(n, sd, per_block_cap):
    return int(lib.lz4mtHipShardPackBound(int(n), ctypes.byref(sd), int(per_block_cap)))


def shard_reset(n, sd, ws, stream=None):
    """Zeroes the round state of ``ws`` on ``stream`` (before every encode, and
    stream-ordered before that call's first pack too)."""
    r = lib.lz4mtHipShardReset(int(n), ctypes.byref(sd), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream(stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipShardReset")


def shard_encode(src, sd, ws, stream=None):
    """Launches the shard's encode (+ block checksums); asynchronous on
    ``stream``.  ``ws`` must have been reset (``shard_reset``) first."""
    _check_dev(src, "src")
    r = lib.lz4mtHipShardEncode(ctypes.c_void_p(src.data_ptr() if src.numel() else ws.data_ptr()), src.numel(),
                                ctypes.byref(sd), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _stream(stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipShardEncode")


def shard_pack(src, sd, ws, pack, per_block_cap, final, stream=None):
    """One round into ``pack``; asynchronous.  The 64-byte header at pack[:64]
    says how many bytes to send (u64 at 24) and whether the shard is complete
    (u32 at 36, bit 0)."""
    r = lib.lz4mtHipShardPack(ctypes.c_void_p(src.data_ptr() if src.numel() else ws.data_ptr()), src.numel(),
                              ctypes.byref(sd), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                              ctypes.c_void_p(pack.data_ptr()), pack.numel(), int(per_block_cap), int(bool(final)),
                              _stream(stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipShardPack")


def shard_unpack(pack, n, sd, mirror, stream=None):
    """A received pack (a tensor, or the device address of one) into ``mirror``."""
    ptr = pack if isinstance(pack, int) else pack.data_ptr()
    r = lib.lz4mtHipShardUnpack(ctypes.c_void_p(ptr), int(n), ctypes.byref(sd),
                                ctypes.c_void_p(mirror.data_ptr()), mirror.numel(), _stream(stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipShardUnpack")


def shard_assemble(src, n, sd, ws, body, stream=None):
    """The shard's records into ``body`` (src: the shard's own source, or None for a mirror)."""
    r = lib.lz4mtHipShardAssemble(ctypes.c_void_p(src.data_ptr() if src is not None and src.numel() else None),
                                  int(n), ctypes.byref(sd), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                  ctypes.c_void_p(body.data_ptr() if body.numel() else None), body.numel(),
                                  _stream(stream))
    if r != Result.OK:
        raise Lz4MtError(r, "lz4mtHipShardAssemble")


def shard_body_bytes(n, sd, ws, stream=None):
    """Record bytes of a complete shard workspace (synchronises ``stream``)."""
    v = int(lib.lz4mtHipShardBodyBytes(int(n), ctypes.byref(sd), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                       _stream(stream)))
    if v == (1 << 64) - 1:
        raise Lz4MtError(Result.ERROR, "lz4mtHipShardBodyBytes")
    return v
