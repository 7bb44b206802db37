"""The LZ4-HC dictionary fixtures (tests/golden/dict_hc_blocks.json and
dict_hc_fuzz.json) are liblz4 1.9.3's answers: where liblz4 is present every
entry is generated again (tests/golden/make_golden_dict_hc.py, which also
asserts its conditions (a) to (d)) and compared with the committed files; the
fixtures' shape -- which dictionaries, chunks, levels and capacities they pin
(tests/dict_hc_cases.py) -- and their size are checked everywhere."""
import ctypes
import importlib.util
import json
import os

import pytest

import dict_hc_cases as H
from conftest import GOLDEN

LIBLZ4 = "/lib/x86_64-linux-gnu/liblz4.so.1"
FILES = ("dict_hc_blocks.json", "dict_hc_fuzz.json")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def blocks():
    return _load(FILES[0])


@pytest.fixture(scope="module")
def fuzz():
    return _load(FILES[1])


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_dict_hc", os.path.join(GOLDEN, "make_golden_dict_hc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixtures_are_what_liblz4_answers(blocks, fuzz):
    if not os.path.exists(LIBLZ4):
        pytest.skip("liblz4 not present")
    if ctypes.CDLL(LIBLZ4).LZ4_versionNumber() != 10903:
        pytest.skip("liblz4 is not 1.9.3")
    gen = _generator()
    fresh = gen.generate()   # asserts (a) .. (d)
    assert {k: v for k, v in fresh.items() if k != "groups"} == {k: v for k, v in blocks.items() if k != "groups"}
    assert len(fresh["groups"]) == len(blocks["groups"])
    for g, h in zip(fresh["groups"], blocks["groups"]):
        assert g["dict"] == h["dict"] and len(g["entries"]) == len(h["entries"])
        for a, b in zip(g["entries"], h["entries"]):
            assert a == b, (g["dict"], a, b)
    assert json.loads(json.dumps(gen.generate_fuzz())) == fuzz


@pytest.mark.parametrize("name", FILES)
def test_fixture_size(name):
    assert os.path.getsize(os.path.join(GOLDEN, name)) < 256 << 10


def test_entries_cover_the_plan(blocks):
    plan = H.plan()
    assert blocks["lz4_version"] == 10903 and len(plan) == len(blocks["groups"])
    for (dspec, items), g in zip(plan, blocks["groups"]):
        assert g["dict"] == dspec
        assert [tuple(e[:3]) for e in g["entries"]] == items
        d = None
        for name, level, capkind, ret, sha in g["entries"]:
            assert 3 <= level <= 12 and capkind in H.CAP_KINDS and ret >= 0 and len(sha) == 40
            if capkind != "bound" or name.startswith(("bd:", "mixed:")):
                n = int(name.split(":")[1])
            else:
                d = H.make_dict(dspec) if d is None else d
                n = len(H.make_chunk(name, d, dspec["seed"]))
            assert ret <= H.cap_of(capkind, n), (dspec, name, level, capkind)
    main = [g for g in blocks["groups"] if g["dict"]["seed"] == 5 and not g["dict"]["run"]]
    assert [g["dict"]["size"] for g in main] == [0, 3, 4, 5, 8, 4096, 65535, 65536, 65537, 100000]
    for g in main:
        by = {}
        for name, level, capkind, _, _ in g["entries"]:
            by.setdefault((name, level), []).append(capkind)
        for n in [0, 1, 12, 13, 64, 1000, 4096, 65535, 70000]:
            for level in (3, 9, 10, 12):
                assert by[(f"bd:{n}", level)] == (["bound", "n", "n-1", "n/3"] if level in (9, 12) else ["bound"])
        for n in (1000, 4096, 70000):
            assert all((f"mixed:{n}", level) in by for level in (3, 9, 10, 12))
        more = sorted({lv for (name, lv) in by if lv in (4, 5, 6, 7, 8, 11)})
        assert more == ([4, 5, 6, 7, 8, 11] if g["dict"]["size"] == 4096 else [])
        assert (("bd:300000", 9) in by) == (g["dict"]["size"] == 65536)
        hand = {name for (name, _) in by if name.startswith(("hand:", "tail:"))}
        want = set(H.C.HAND) | {f"tail:{k}" for k in (1, 2, 3, 4, 5, 6, 7, 40, 300)}
        assert hand == (want if g["dict"]["size"] in (4096, 65536) else set())
    runs = [g for g in blocks["groups"] if g["dict"]["run"]]
    assert sorted((g["dict"]["size"], g["dict"]["run"]) for g in runs) == \
        sorted((s, r) for s in (4096, 65536) for r in (1, 2, 3, 4, 8, 50))
    for g in runs:
        assert {e[0] for e in g["entries"]} == {f"run:{n}" for n in (3, 10, 100, 1000)}


def test_a_concatenating_encoder_cannot_pass(blocks):
    """Condition (c), recorded by the generator: at each main level at least 10 entries whose
    bytes differ from liblz4's prefix mode (dictionary and chunk adjacent in one buffer)."""
    assert set(blocks["prefix_differs"]) == {"3", "9", "10", "12"}
    assert all(v >= 10 for v in blocks["prefix_differs"].values()), blocks["prefix_differs"]


def test_short_dictionaries_are_no_dictionary(blocks):
    """Condition (d): below 4 bytes nothing is inserted, and liblz4 answers as without a dictionary
    (recorded by the generator from LZ4_compress_HC); so the groups of 0 and 3 bytes agree."""
    assert blocks["short_dict_is_no_dict"] is True
    by = {g["dict"]["size"]: g for g in blocks["groups"] if g["dict"]["seed"] == 5 and not g["dict"]["run"]}
    assert [e[3:] for e in by[0]["entries"]] == [e[3:] for e in by[3]["entries"]]


def test_the_dictionary_shows_in_the_fixture(blocks):
    by = {g["dict"]["size"]: g for g in blocks["groups"] if g["dict"]["seed"] == 5 and not g["dict"]["run"]}

    def ret(size, n, level):
        return next(e[3] for e in by[size]["entries"] if e[:3] == [f"bd:{n}", level, "bound"])
    for size in (4096, 65535, 65536, 65537, 100000):
        for n in (1000, 4096):
            for level in (3, 9, 10, 12):
                assert 0 < ret(size, n, level) < ret(0, n, level), (size, n, level)


def test_fuzz_cases_cover_the_plan(fuzz):
    plan = H.fuzz_plan()
    assert fuzz["lz4_version"] == 10903 and fuzz["dicts"] == H.FUZZ_DICTS
    assert len(plan) == len(fuzz["cases"]) == H.FUZZ_N
    assert [tuple(c[:6]) for c in fuzz["cases"]] == plan
    assert {c[4] for c in fuzz["cases"]} == set(range(3, 13))
    assert all(c[2] <= 20000 and 0 <= c[6] <= H.cap_of(c[5], c[2]) and len(c[7]) == 40 for c in fuzz["cases"])
