"""Pins the oracle's two dictionary operations (orc_lz4_compress_dict,
orc_lz4_decompress_safe_usingDict) and checks the inputs of the GPU tests
that lean on them -- all on the CPU.

  1. the fixture tests/golden/dict_blocks.json (liblz4 1.9.3's own answers): every
     compress and decode entry, on every host
  2. liblz4 itself where it is present: a differential fuzz of both functions
  3. the block synthesizer (lz4_synth.py): the oracle decodes every valid block of the fixed
     batches (synth_cases.py) to the plain text the synthesizer computed byte by byte, with the
     dictionary and without, rejects every invalid one, and the batches hold every class
"""
import ctypes
import hashlib
import json
import os
import random

import pytest

import dict_cases as C
import lz4_synth as S
import oracle
import synth_cases as K
from conftest import GOLDEN

LIBLZ4 = "/lib/x86_64-linux-gnu/liblz4.so.1"


def sha1(b):
    return hashlib.sha1(b).hexdigest()


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "dict_blocks.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------------------
# 1. the fixture
# ---------------------------------------------------------------------------
def test_compress_dict_vs_fixture(fixture):
    n = 0
    for g in fixture["compress"]:
        d = C.make_dict(g["dict"])
        for e in g["entries"]:
            blk = oracle.compress_block_dict(d, C.make_chunk(e["chunk"], d), e["cap"])
            assert len(blk) == e["ret"] and sha1(blk) == e["sha1"], (g["dict"], e)
            n += 1
    assert n == 590


def test_decompress_dict_vs_fixture(fixture):
    n = 0
    for g in fixture["decode"]:
        d = C.make_dict(g["dict"])[g["front"]:] if g["use"] else b""
        for e in g["entries"]:
            ret, out = oracle.decompress_block_dict(bytes.fromhex(e["block"]), e["cap"], d)
            assert ret == e["ret"], (g["dict"], g["front"], g["use"], e["name"], ret)
            if ret >= 0:
                assert sha1(out) == e["sha1"], e["name"]
            n += 1
    assert n == 37


def test_without_a_dictionary_the_decoder_is_the_plain_one():
    rnd = random.Random(3)
    for blk, plain, _, _ in K.synth_batch(0)[0][:20]:
        for cap in (len(plain), len(plain) - 1, rnd.randrange(len(plain))):
            assert oracle.decompress_block_dict(blk, cap, b"") == oracle.decompress_block(blk, cap)


# ---------------------------------------------------------------------------
# 2. liblz4 1.9.3 itself
# ---------------------------------------------------------------------------
def _liblz4():
    if not os.path.exists(LIBLZ4):
        pytest.skip("liblz4 not present")
    lz = ctypes.CDLL(LIBLZ4)
    if lz.LZ4_versionNumber() != 10903:
        pytest.skip("liblz4 is not 1.9.3")
    lz.LZ4_createStream.restype = ctypes.c_void_p
    lz.LZ4_freeStream.argtypes = [ctypes.c_void_p]
    lz.LZ4_loadDict.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lz.LZ4_compress_fast_continue.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int]
    lz.LZ4_decompress_safe_usingDict.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_int]
    return lz


def _own(data):
    """A buffer of its own, one byte longer than ``data``: nothing starts where it ends."""
    return ctypes.create_string_buffer(bytes(data), len(data) + 1)


def lz_compress(lz, db, dlen, src, cap):
    st = lz.LZ4_createStream()
    ob = ctypes.create_string_buffer(cap + 64)
    lz.LZ4_loadDict(st, db, dlen)
    n = lz.LZ4_compress_fast_continue(st, _own(src), ob, len(src), cap, 1)
    lz.LZ4_freeStream(st)
    return ob.raw[:n]


def lz_decompress(lz, db, dlen, block, cap):
    ob = ctypes.create_string_buffer(cap + 64)
    n = lz.LZ4_decompress_safe_usingDict(_own(block), ob, len(block), cap, db, dlen)
    return n, (ob.raw[:n] if n > 0 else b"")


def test_differential_vs_liblz4():
    """Both functions against the library, on the encode fuzz's dictionaries and chunks: same return
    value, same bytes -- then every block damaged, at several capacities and dictionary sizes."""
    lz = _liblz4()
    for size, seed in [(size, seed) for size in K.FUZZ_DICTS for seed in (0, 1, 2)]:
        d = K.fuzz_dict(size, seed)
        db = _own(d)
        rnd = random.Random(size + seed)
        others = [(b"", _own(b"")), (d[-9:], _own(d[-9:])), (d[1:], _own(d[1:]))]
        for src in K.fuzz_chunks(size, seed):
            n = len(src)
            blk = None
            for cap in K.caps_of(rnd, n):
                want = lz_compress(lz, db, len(d), src, cap)
                assert oracle.compress_block_dict(d, src, cap) == want, (size, n, cap)
                blk = blk or want
            assert blk and lz_decompress(lz, db, len(d), blk, n) == (n, src if n else b"")
            variants = [blk] + (S.damaged(rnd, blk) if n <= 20000 else S.damaged(rnd, blk)[:3])
            for v in variants:
                for cap in (0, n - 1, n, n + 100, rnd.randrange(n + 1)):
                    if cap < 0:
                        continue
                    for dd, ddb in [(d, db)] + others[:1 if n > 20000 else 3]:
                        want = lz_decompress(lz, ddb, len(dd), v, cap)
                        got = oracle.decompress_block_dict(v, cap, dd)
                        assert got[0] == want[0], (size, n, cap, len(dd), got[0], want[0])
                        assert got[1] == want[1], (size, n, cap, len(dd))


def test_synthesized_blocks_vs_liblz4():
    """liblz4 accepts every block the synthesizer calls valid and decodes it to the synthesizer's
    plain text; what it answers for the invalid ones, and at capacity n - 1, is the oracle's."""
    lz = _liblz4()
    for size in [0] + K.SYNTH_DICTS:
        d = K.synth_dict(size)
        db = _own(d)
        for i, (blk, plain, prof, _) in enumerate(K.synth_batch(size)[0]):
            if plain is None:
                want = lz_decompress(lz, db, len(d), blk, 100000)
                assert want[0] < 0 and oracle.decompress_block_dict(blk, 100000, d) == want, (size, i)
                continue
            n = len(plain)
            assert lz_decompress(lz, db, len(d), blk, n) == (n, plain), (size, i, prof)
            assert oracle.decompress_block_dict(blk, n - 1, d) == lz_decompress(lz, db, len(d), blk, n - 1)


# ---------------------------------------------------------------------------
# 3. the synthesizer and the fixed batches of the GPU tests
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", [0] + K.SYNTH_DICTS)
def test_oracle_decodes_synthesized_blocks(size):
    d = K.synth_dict(size)
    blocks, _ = K.synth_batch(size)
    valid = [b for b in blocks if b.plain is not None]
    assert len(valid) == K.N_BLOCKS
    assert min(len(b.plain) for b in valid) < 400 and 80000 < max(len(b.plain) for b in valid) < 90000
    for i, (blk, plain, prof, _) in enumerate(valid):
        n = len(plain)
        for cap in (n, n + 1, n + 100):
            assert oracle.decompress_block_dict(blk, cap, d) == (n, plain), (size, i, prof, cap)
        assert oracle.decompress_block_dict(blk, n - 1, d)[0] < 0, (size, i)
    invalid = [b for b in blocks if b.plain is None]
    assert len(invalid) == (K.N_INVALID if size == 0 or size in K.INVALID_DICTS else 0)
    for i, (blk, _, _, _) in enumerate(invalid):
        assert oracle.decompress_block_dict(blk, 100000, d)[0] < 0, (size, i)
    if size == 0:
        for blk, plain, _, _ in valid:
            assert oracle.decompress_block(blk, len(plain)) == (len(plain), plain)
        for blk, _, _, _ in invalid:
            assert oracle.decompress_block(blk, 100000)[0] < 0


def test_blocks_that_need_the_dictionary_fail_without_it():
    """The dictionary matters to the synthesized blocks: without it (or one byte short) they are refused."""
    for size in (8, 4096, 65536):
        d = K.synth_dict(size)
        valid = [b for b in K.synth_batch(size)[0]
                 if b.plain is not None and b.stats[("forced", "low", b.profile["low"])]]
        assert len(valid) > K.N_BLOCKS // 2
        first = [b for b in valid if b.profile.get("low") == "first_byte"]
        assert all(oracle.decompress_block_dict(b.block, len(b.plain), b"")[0] < 0 for b in valid)
        if size < 65536:   # with 64 KiB and more no offset reaches the first byte, and none is checked
            assert first and all(oracle.decompress_block_dict(b.block, len(b.plain), d[1:])[0] < 0 for b in first)


def test_invalid_dictionaries_are_the_ones_an_offset_can_miss():
    assert K.INVALID_DICTS == [8, 9, 63, 64, 4096, 16384]


@pytest.mark.parametrize("size", [0] + K.SYNTH_DICTS)
def test_fixed_batches_hold_every_class(size):
    _, stats = K.synth_batch(size)
    missing = [k for k in K.required_classes(size) if stats[k] < 1]
    assert not missing, (size, missing)
    if size:
        forced = {k: v for k, v in stats.items() if k[0] == "forced"}
        # every class asked for at P < 64 fitted in at least one block
        lows = {k[2] for k, v in forced.items() if k[1] == "low" and v}
        want = set(S.DICT_CLASSES) - ({"off_65535"} if size < S.MAX_OFF else {"first_byte"} if size > S.MAX_OFF
                                      else set())
        assert lows == want, (size, lows)


def test_required_classes_name_everything_the_synthesizer_counts():
    need = set(K.required_classes(4096))
    assert {k[1] for k in need if k[0] == "off"} == set(S.OFF_CLASSES)
    assert {k[2] for k in need if k[0] == "dict" and k[1] == "low"} == set(S.DICT_CLASSES) - {"off_65535"}
    assert {k[2] for k in need if k[0] == "dict" and k[1] == "high"} == set(S.DICT_CLASSES) - {"off_65535", "off1..7"}
    need = set(K.required_classes(65536))
    assert ("dict", "low", "off_65535") in need and ("dict", "high", "off_65535") in need


def test_runs_are_longer_than_the_far_table():
    """A far or dictionary run has RUN_MIN sequences or more in a row (the decoder's far table takes 8
    per batch); counted from the block itself, not from stats."""
    assert S.RUN_MIN >= 16
    rnd = random.Random(1)
    d = K.synth_dict(4096)
    for _ in range(20):
        w = S._Writer(rnd, d)
        S._grow(w, 16400)
        before = w.stats["sequences"]
        S._run_far(w)
        S._run_dict(w)
        assert w.stats["sequences"] - before >= 2 * S.RUN_MIN
        blk, plain, _ = w.finish()
        assert oracle.decompress_block_dict(blk, len(plain), d) == (len(plain), plain)


# ---------------------------------------------------------------------------
# the encode fuzz's inputs
# ---------------------------------------------------------------------------
def test_fuzz_sources_reach_the_dictionary():
    """The chunks of the encode fuzz are what they are meant to be: with the dictionary their blocks
    hold matches below position 0 (they do not decode without it), and round-trip with it."""
    for size in (12, 4096, 65536, 100000):
        d = K.fuzz_dict(size)
        assert len(d) == size
        chunks = K.fuzz_chunks(size)
        assert [len(c) for c in chunks[:len(K.FUZZ_SIZES)]] == K.FUZZ_SIZES
        needs = 0
        for c in chunks:
            blk = oracle.compress_block_dict(d, c)
            assert blk and oracle.decompress_block_dict(blk, len(c), d) == (len(c), c if c else b"")
            needs += oracle.decompress_block_dict(blk, len(c), b"")[0] < 0
        assert needs >= (1 if size == 12 else 10), (size, needs)
    hand = K.fuzz_chunks(4096)[-1]
    d = K.fuzz_dict(4096)
    assert len(hand) == 20240 and hand[20000:20040] == d[-40:] and hand[20040:] == hand[:200]


def test_oracle_library_is_rebuilt_when_a_source_is_newer():
    src = os.path.join(oracle.HERE, "lz4_oracle.c")
    assert not oracle._stale()
    old = os.stat(oracle.LIB_PATH)
    try:
        os.utime(oracle.LIB_PATH, (old.st_atime, os.path.getmtime(src) - 10))
        assert oracle._stale()
    finally:
        os.utime(oracle.LIB_PATH, (old.st_atime, old.st_mtime))
