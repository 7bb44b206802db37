"""The dictionary fixture (tests/golden/dict_blocks.json) is liblz4 1.9.3's
answer: where liblz4 is present every entry is generated again
(tests/golden/make_golden_dict.py) and compared with the committed file; the
fixture's shape -- which dictionaries, chunks and capacities it pins
(tests/dict_cases.py) -- is checked everywhere."""
import ctypes
import importlib.util
import json
import os

import pytest

import dict_cases as C
from conftest import GOLDEN

LIBLZ4 = "/lib/x86_64-linux-gnu/liblz4.so.1"


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "dict_blocks.json")) as f:
        return json.load(f)


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_dict", os.path.join(GOLDEN, "make_golden_dict.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_what_liblz4_answers(fixture):
    if not os.path.exists(LIBLZ4):
        pytest.skip("liblz4 not present")
    if ctypes.CDLL(LIBLZ4).LZ4_versionNumber() != 10903:
        pytest.skip("liblz4 is not 1.9.3")
    fresh = _generator().generate()
    assert fresh["lz4_version"] == fixture["lz4_version"] == 10903
    for part in ("compress", "decode"):
        assert len(fresh[part]) == len(fixture[part]), part
        for g, h in zip(fresh[part], fixture[part]):
            assert {k: v for k, v in g.items() if k != "entries"} == {k: v for k, v in h.items() if k != "entries"}
            assert len(g["entries"]) == len(h["entries"]), g["dict"]
            for a, b in zip(g["entries"], h["entries"]):
                assert a == b, (part, g["dict"], a, b)


def test_fixture_size():
    assert os.path.getsize(os.path.join(GOLDEN, "dict_blocks.json")) < 256 << 10


def test_compress_entries_cover_the_plan(fixture):
    plan = C.compress_plan()
    assert len(plan) == len(fixture["compress"])
    for (dspec, items), g in zip(plan, fixture["compress"]):
        assert g["dict"] == dspec
        assert [(e["chunk"], e["capkind"]) for e in g["entries"]] == [(c, k) for c, k in items]
        for e in g["entries"]:
            assert e["cap"] == C.cap_of(e["capkind"], e["chunk"]["n"])
            assert 0 <= e["ret"] <= e["cap"] and len(e["sha1"]) == 40
    main = [g for g in fixture["compress"] if g["dict"]["seed"] == C.DICT_SEED]
    assert [g["dict"]["size"] for g in main] == [0, 7, 8, 9, 10, 11, 4096, 65535, 65536, 65537, 100000]
    for g in main:
        text = sorted({e["chunk"]["n"] for e in g["entries"] if e["chunk"]["kind"] == "bd"})
        want = [0, 1, 12, 13, 64, 1000, 4096, 65535, 70000] + ([300000] if g["dict"]["size"] == 65536 else [])
        assert text == want, g["dict"]
        for n in want:
            kinds = [e["capkind"] for e in g["entries"] if e["chunk"]["kind"] == "bd" and e["chunk"]["n"] == n]
            assert kinds == ["bound", "n", "n-1", "n/3"]
        hand = {e["chunk"]["kind"] for e in g["entries"] if e["chunk"]["kind"].startswith("hand:")}
        assert hand == (set(C.HAND) if g["dict"]["size"] in (4096, 65536) else set())
    # the graph test's further dictionaries of 4096 bytes
    assert [g["dict"] for g in fixture["compress"][len(main):]] == \
        [{"kind": "bd", "size": 4096, "seed": s} for s in C.GRAPH_SEEDS]


def test_dictionary_sizes_below_8_are_no_dictionary(fixture):
    """HASH_UNIT is 8: dictionaries of 0 and 7 bytes leave the same bytes; 8 to 11 bytes are
    a dictionary (they change dictSmall's limit), whether or not a match is found in them."""
    by = {g["dict"]["size"]: g for g in fixture["compress"] if g["dict"]["seed"] == C.DICT_SEED}
    assert [(e["ret"], e["sha1"]) for e in by[0]["entries"]] == [(e["ret"], e["sha1"]) for e in by[7]["entries"]]


def test_the_dictionary_shows_in_the_fixture(fixture):
    by = {g["dict"]["size"]: g for g in fixture["compress"] if g["dict"]["seed"] == C.DICT_SEED}

    def ret(size, n):
        return next(e["ret"] for e in by[size]["entries"]
                    if e["chunk"]["kind"] == "bd" and e["chunk"]["n"] == n and e["capkind"] == "bound")
    for size in (4096, 65535, 65536, 65537, 100000):
        for n in (1000, 4096):
            assert 0 < ret(size, n) < ret(0, n), (size, n)
    # the trim: 65537 and 100000 bytes keep other last 64 KiB than 65536 bytes of the same text
    assert len({ret(s, 4096) for s in (65536, 65537, 100000)}) == 3


def test_decode_entries(fixture):
    groups = fixture["decode"]
    names = {(g["dict"]["size"], g["front"], g["use"], e["name"]): e for g in groups for e in g["entries"]}
    for g in groups:
        for e in g["entries"]:
            assert len(bytes.fromhex(e["block"])) <= 1100 and e["cap"] <= 1100
            assert ("sha1" in e) == (e["ret"] >= 0)
    assert names[(4096, 0, True, "valid:text")]["ret"] == 1000
    assert names[(4096, 0, True, "valid:hand:over_end")]["ret"] == 320
    for k in ("trunc1", "trunc3", "cap-1", "offset_below_dict_start", "offset_below_dict_start_long"):
        assert names[(4096, 0, True, k)]["ret"] < 0, k
    assert names[(4096, 0, True, "offset_at_dict_start")]["ret"] == 16
    assert names[(4096, 0, True, "offset_at_dict_start_long")]["ret"] == 108
    assert names[(4096, 0, False, "nodict:text")]["ret"] < 0
    assert names[(4096, 100, True, "short:text")]["ret"] < 0
    assert names[(9, 0, True, "offset_below_dict_start")]["ret"] < 0
    assert names[(65536, 0, True, "offset_65535")]["ret"] == 16
