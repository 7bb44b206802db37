"""Generates tests/golden/dict_blocks.json: liblz4 1.9.3's own answers for the
batched dictionary operators (include/lz4mt_hip.h section 5b).

Source: liblz4.so.1 (LZ4_versionNumber() == 10903) through ctypes, with the
dictionary, the source and the destination in separate buffers, none adjacent
to another (lz4's usingExtDict / forceExtDict modes):

  compress    LZ4_loadDict(stream, dict, dictSize);
              LZ4_compress_fast_continue(stream, src, dst, n, cap, 1);
  decompress  LZ4_decompress_safe_usingDict(src, dst, n, cap, dict, dictSize);

The cases and their inputs are tests/dict_cases.py's.

Run:  python tests/golden/make_golden_dict.py   (rewrites the fixture)
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import dict_cases as C  # noqa: E402

LIBLZ4 = "/lib/x86_64-linux-gnu/liblz4.so.1"
OUT = os.path.join(HERE, "dict_blocks.json")


def load_lz4():
    lz = ctypes.CDLL(LIBLZ4)
    assert lz.LZ4_versionNumber() == 10903, lz.LZ4_versionNumber()
    lz.LZ4_createStream.restype = ctypes.c_void_p
    lz.LZ4_freeStream.argtypes = [ctypes.c_void_p]
    lz.LZ4_loadDict.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lz.LZ4_compress_fast_continue.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int]
    lz.LZ4_decompress_safe_usingDict.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_int]
    return lz


def _buf(data):
    """A buffer of its own, one byte longer than ``data``: nothing can start where it ends."""
    return ctypes.create_string_buffer(bytes(data), len(data) + 1)


def compress(lz, d, src, cap):
    """The block (b"" when it does not fit): a new stream per chunk, as the batch call gives every chunk."""
    st = lz.LZ4_createStream()
    db, sb, ob = _buf(d), _buf(src), ctypes.create_string_buffer(cap + 64)
    lz.LZ4_loadDict(st, db, len(d))
    n = lz.LZ4_compress_fast_continue(st, sb, ob, len(src), cap, 1)
    lz.LZ4_freeStream(st)
    assert 0 <= n <= cap
    return ob.raw[:n]


def decompress(lz, d, block, cap):
    db, sb, ob = _buf(d), _buf(block), ctypes.create_string_buffer(cap + 64)
    n = lz.LZ4_decompress_safe_usingDict(sb, ob, len(block), cap, db, len(d))
    return n, (ob.raw[:n] if n > 0 else b"")


def sha1(b):
    return hashlib.sha1(b).hexdigest()


def compress_groups(lz):
    groups = []
    for dspec, items in C.compress_plan():
        d = C.make_dict(dspec)
        entries = []
        for cspec, capkind in items:
            src = C.make_chunk(cspec, d)
            cap = C.cap_of(capkind, len(src))
            blk = compress(lz, d, src, cap)
            if blk:
                assert decompress(lz, d, blk, len(src)) == (len(src), src) or not src
            entries.append({"chunk": cspec, "capkind": capkind, "cap": cap, "ret": len(blk), "sha1": sha1(blk)})
        groups.append({"dict": dspec, "entries": entries})
        # the fixture must show that the dictionary is used: word-like chunks come out shorter with it
        if dspec["size"] >= 4096:
            for n in (1000, 4096):
                cspec = {"kind": "bd", "n": n, "seed": dspec["seed"], "skip": C.CHUNK_SKIP}
                src = C.make_chunk(cspec, d)
                with_d, without = compress(lz, d, src, C.bound(n)), compress(lz, b"", src, C.bound(n))
                assert len(with_d) < len(without), (dspec, n, len(with_d), len(without))
    return groups


def crafted(offset, tail):
    """4 literals, a 4-byte match at ``offset``, then ``tail`` last literals."""
    lits = bytes(range(0x61, 0x61 + 26)) * 8
    tok = bytes([min(tail, 15) << 4]) + (bytes([tail - 15]) if tail >= 15 else b"")
    assert tail < 15 + 255
    return bytes([0x40]) + b"abcd" + offset.to_bytes(2, "little") + tok + lits[:tail]


def decode_groups(lz):
    text = {"kind": "bd", "n": 1000, "seed": C.DICT_SEED, "skip": C.CHUNK_SKIP}
    groups = []

    def group(dsize, front, use, entries):
        dspec = {"kind": "bd", "size": dsize, "seed": C.DICT_SEED}
        d = C.make_dict(dspec)[front:] if use else b""
        out = []
        for name, blk, cap in entries:
            ret, data = decompress(lz, d, blk, cap)
            e = {"name": name, "block": blk.hex(), "cap": cap, "ret": ret}
            if ret >= 0:
                e["sha1"] = sha1(data)
            out.append(e)
        groups.append({"dict": dspec, "front": front, "use": use, "entries": out})
        return out

    def blocks_for(dsize, kinds):
        d = C.make_dict({"kind": "bd", "size": dsize, "seed": C.DICT_SEED})
        res = []
        for k in kinds:
            src = C.make_chunk(text, d) if k == "text" else C.hand_chunk(k, d)
            assert len(src) <= 1024
            res.append((k, src, compress(lz, d, src, C.bound(len(src)))))
        return res

    b4k = blocks_for(4096, ["text"] + C.HAND)
    tname, tsrc, tblk = b4k[0]
    over = b4k[1][2]
    ents = [(f"valid:{k}", blk, len(src)) for k, src, blk in b4k]
    ents += [("trunc1", tblk[:-1], len(tsrc)), ("trunc3", tblk[:-3], len(tsrc)),
             ("cap-1", tblk, len(tsrc) - 1), ("cap+100", tblk, len(tsrc) + 100), ("cap0", tblk, 0),
             ("offset_at_dict_start", crafted(4 + 4096, 8), 16), ("offset_below_dict_start", crafted(4 + 4097, 8), 16),
             ("offset_at_dict_start_long", crafted(4 + 4096, 100), 108),
             ("offset_below_dict_start_long", crafted(4 + 4097, 100), 108)]
    got = group(4096, 0, True, ents)
    by = {e["name"]: e for e in got}
    assert all(by[f"valid:{k}"]["ret"] == len(src) for k, src, _ in b4k)
    assert by["offset_at_dict_start"]["ret"] == 16 and by["offset_below_dict_start"]["ret"] < 0
    assert by["offset_at_dict_start_long"]["ret"] == 108 and by["offset_below_dict_start_long"]["ret"] < 0
    assert by["trunc1"]["ret"] < 0 and by["trunc3"]["ret"] < 0 and by["cap-1"]["ret"] < 0
    # a match that starts in the dictionary and is longer than what remains there
    assert decompress(lz, b"", over, 320)[0] < 0
    # the same blocks without the dictionary, and with its first 100 bytes missing
    same = [("nodict:text", tblk, len(tsrc)), ("nodict:over_end", over, 320)]
    group(4096, 0, False, same)
    group(4096, 100, True, [("short:text", tblk, len(tsrc)), ("short:over_end", over, 320),
                            ("short:dict_start", b4k[2][2], len(b4k[2][1]))])
    # 64 KiB and more: no offset check (an offset reaches 65535 at most)
    for dsize in (65536, 100000):
        bs = blocks_for(dsize, ["text", "hand:over_end", "hand:dict_start"])
        got = group(dsize, 0, True, [(f"valid:{k}", blk, len(src)) for k, src, blk in bs] +
                    [("offset_65535", crafted(65535, 8), 16), ("offset_65535_long", crafted(65535, 100), 108)])
        assert all(e["ret"] >= 0 for e in got)
    # the largest dictionary whose offsets are checked (none can reach below it from the block's first bytes)
    bs = blocks_for(65535, ["text", "hand:over_end"])
    got = group(65535, 0, True, [(f"valid:{k}", blk, len(src)) for k, src, blk in bs] +
                [("offset_65535", crafted(65535, 8), 16)])
    assert all(e["ret"] >= 0 for e in got)
    # the smallest dictionary that counts
    bs = blocks_for(9, ["text"])
    got = group(9, 0, True, [(f"valid:{k}", blk, len(src)) for k, src, blk in bs] +
                [("offset_at_dict_start", crafted(4 + 9, 8), 16), ("offset_below_dict_start", crafted(4 + 10, 8), 16),
                 ("offset_below_dict_start_long", crafted(4 + 10, 100), 108)])
    assert [e["ret"] >= 0 for e in got] == [True, True, False, False]
    return groups


def generate():
    lz = load_lz4()
    return {"lz4_version": 10903, "compress": compress_groups(lz), "decode": decode_groups(lz)}


def main():
    fx = generate()
    with open(OUT, "w") as f:
        json.dump(fx, f, separators=(",", ":"))
        f.write("\n")
    n = sum(len(g["entries"]) for g in fx["compress"]), sum(len(g["entries"]) for g in fx["decode"])
    print(f"{OUT}: {n[0]} compress entries, {n[1]} decode entries, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
