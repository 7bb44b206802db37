"""Generates tests/golden/dict_hc_blocks.json and dict_hc_fuzz.json: liblz4
1.9.3's own answers for the batched LZ4-HC compress with a shared dictionary
(include/lz4mt_hip.h section 5c).

Source: liblz4.so.1 (LZ4_versionNumber() == 10903) through ctypes.  Every chunk
takes a fresh LZ4_createStreamHC() stream, with the dictionary, the source and
the destination in separate buffers, none adjacent to another (lz4hc's
external-dictionary mode):

  LZ4_resetStreamHC_fast(s, level);
  LZ4_loadDictHC(s, dict, dictSize);
  LZ4_compress_HC_continue(s, src, dst, n, cap);

The cases and their inputs are tests/dict_hc_cases.py's.  An entry is
[chunk name, level, cap kind, ret, sha1 of the block].  The generator asserts:

  (a) every block decodes back through LZ4_decompress_safe_usingDict;
  (b) at dictionaries of 4096 bytes and more the word-like chunks come out
      shorter than without the dictionary;
  (c) at each of levels 3, 9, 10 and 12 at least 10 entries differ from
      liblz4's prefix mode (the same data with dictionary and chunk adjacent
      in one buffer): a kernel that concatenates the two cannot pass.  The
      counts are recorded ("prefix_differs");
  (d) whether dictionaries shorter than 4 bytes give the bytes of
      LZ4_compress_HC without a dictionary: recorded ("short_dict_is_no_dict")
      and asserted to hold.

Run:  python tests/golden/make_golden_dict_hc.py   (rewrites both fixtures)
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import dict_hc_cases as H  # noqa: E402

LIBLZ4 = "/lib/x86_64-linux-gnu/liblz4.so.1"
OUT = os.path.join(HERE, "dict_hc_blocks.json")
OUT_FUZZ = os.path.join(HERE, "dict_hc_fuzz.json")


def load_lz4():
    lz = ctypes.CDLL(LIBLZ4)
    assert lz.LZ4_versionNumber() == 10903, lz.LZ4_versionNumber()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lz.LZ4_createStreamHC.restype = vp
    lz.LZ4_freeStreamHC.argtypes = [vp]
    lz.LZ4_resetStreamHC_fast.argtypes = [vp, ci]
    lz.LZ4_loadDictHC.argtypes = [vp, vp, ci]
    lz.LZ4_compress_HC_continue.argtypes = [vp, vp, vp, ci, ci]
    lz.LZ4_compress_HC.argtypes = [vp, vp, ci, ci, ci]
    lz.LZ4_decompress_safe_usingDict.argtypes = [vp, vp, ci, ci, vp, ci]
    return lz


def _buf(data):
    """A buffer of its own, one byte longer than ``data``: nothing can start where it ends."""
    return ctypes.create_string_buffer(bytes(data), len(data) + 1)


def compress(lz, d, src, cap, level):
    """The block (b"" when it does not fit): a new stream per chunk, as the batch call gives every chunk."""
    st = lz.LZ4_createStreamHC()
    db, sb, ob = _buf(d), _buf(src), ctypes.create_string_buffer(cap + 64)
    lz.LZ4_resetStreamHC_fast(st, level)
    lz.LZ4_loadDictHC(st, db, len(d))
    n = lz.LZ4_compress_HC_continue(st, sb, ob, len(src), cap)
    lz.LZ4_freeStreamHC(st)
    assert 0 <= n <= cap
    return ob.raw[:n]


def compress_prefix(lz, d, src, cap, level):
    """The same calls with the chunk right behind the dictionary in one buffer: lz4hc's prefix mode."""
    st = lz.LZ4_createStreamHC()
    both, ob = _buf(bytes(d) + bytes(src)), ctypes.create_string_buffer(cap + 64)
    base = ctypes.addressof(both)
    lz.LZ4_resetStreamHC_fast(st, level)
    lz.LZ4_loadDictHC(st, base, len(d))
    n = lz.LZ4_compress_HC_continue(st, base + len(d), ob, len(src), cap)
    lz.LZ4_freeStreamHC(st)
    return ob.raw[:max(n, 0)]


def compress_nodict(lz, src, cap, level):
    sb, ob = _buf(src), ctypes.create_string_buffer(cap + 64)
    n = lz.LZ4_compress_HC(sb, ob, len(src), cap, level)
    return ob.raw[:max(n, 0)]


def decompress(lz, d, block, cap):
    db, sb, ob = _buf(d), _buf(block), ctypes.create_string_buffer(cap + 64)
    n = lz.LZ4_decompress_safe_usingDict(sb, ob, len(block), cap, db, len(d))
    return n, (ob.raw[:n] if n > 0 else b"")


def sha1(b):
    return hashlib.sha1(b).hexdigest()


def block_groups(lz):
    groups, differs, short_same = [], {str(lv): 0 for lv in H.LEVELS_MAIN}, True
    for dspec, items in H.plan():
        d = H.make_dict(dspec)
        entries = []
        for name, level, capkind in items:
            src = H.make_chunk(name, d, dspec["seed"])
            cap = H.cap_of(capkind, len(src))
            blk = compress(lz, d, src, cap, level)
            if blk:   # (a)
                assert decompress(lz, d, blk, len(src)) == (len(src), src) or not src, (dspec, name, level)
            if str(level) in differs and compress_prefix(lz, d, src, cap, level) != blk:
                differs[str(level)] += 1
            if len(d) < 4 and compress_nodict(lz, src, cap, level) != blk:   # (d)
                short_same = False
            entries.append([name, level, capkind, len(blk), sha1(blk)])
        groups.append({"dict": dspec, "entries": entries})
        if dspec["size"] >= 4096 and not dspec["run"]:   # (b)
            for level in H.LEVELS_MAIN:
                for n in (1000, 4096):
                    src = H.make_chunk(f"bd:{n}", d, dspec["seed"])
                    with_d = compress(lz, d, src, H.bound(n), level)
                    assert len(with_d) < len(compress_nodict(lz, src, H.bound(n), level)), (dspec, n, level)
    assert all(v >= 10 for v in differs.values()), differs   # (c)
    assert short_same   # (d): the header's contract for dictionaries below 4 bytes
    return groups, differs, short_same


def fuzz_cases(lz):
    dicts = [H.make_dict(s) for s in H.FUZZ_DICTS]
    out = []
    for di, kind, n, seed, level, capkind in H.fuzz_plan():
        src = H.fuzz_chunk(kind, n, seed, dicts[di])
        cap = H.cap_of(capkind, n)
        blk = compress(lz, dicts[di], src, cap, level)
        if blk:
            assert decompress(lz, dicts[di], blk, n) == (n, src) or not src
        out.append([di, kind, n, seed, level, capkind, len(blk), sha1(blk)])
    return out


def generate():
    lz = load_lz4()
    groups, differs, short_same = block_groups(lz)
    return {"lz4_version": 10903, "groups": groups, "prefix_differs": differs, "short_dict_is_no_dict": short_same}


def generate_fuzz():
    return {"lz4_version": 10903, "dicts": H.FUZZ_DICTS, "cases": fuzz_cases(load_lz4())}


def main():
    for path, fx, key in ((OUT, generate(), "groups"), (OUT_FUZZ, generate_fuzz(), "cases")):
        with open(path, "w") as f:
            json.dump(fx, f, separators=(",", ":"))
            f.write("\n")
        n = sum(len(g["entries"]) for g in fx[key]) if key == "groups" else len(fx[key])
        print(f"{path}: {n} entries, {os.path.getsize(path)} bytes", {k: v for k, v in fx.items() if k.startswith(("prefix", "short"))})


if __name__ == "__main__":
    main()
