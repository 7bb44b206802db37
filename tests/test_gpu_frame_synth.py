"""The frame decoders on synthesized frames (lz4_frame_synth.py, the fixed
frames of frame_synth_cases.py): linked (-BD) frames of short, stored and
empty blocks, more blocks than one scan pass of k_dlink_plan, chains longer
than the rounds, sources three and ten blocks back, batches that decode less
than the 64 KiB window, blocks of exactly blockMax; frames of independent
blocks whose records lie a few bytes apart and whose blocks no encoder writes.

Everything is bit-exact.  The expected bytes of a valid frame are the
builder's text: no decoder computed them.  Result codes and the bytes written
before an error are the oracle's, and equal the text of the blocks before the
failing one (tests/test_frame_synth.py asserts both on the CPU, with the
conditions on the inputs).
"""
import random

import pytest
import torch

import frame_synth_cases as C
import lz4_frame_synth as F
import oracle

pytestmark = pytest.mark.gpu

L = None
FILL = 0xA5
MODES = ["DEVICE", "PARALLEL", "SEQUENTIAL"]


@pytest.fixture(scope="module", autouse=True)
def lib():
    global L
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import lz4mt_amd
    L = lz4mt_amd
    assert L.device_count() > 0
    return L


def dev(b):
    t = torch.empty(max(len(b), 1), dtype=torch.uint8, device="cuda")
    if b:
        t[:len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return t[:len(b)]


def host(t):
    return bytes(t.cpu().numpy().tobytes())


def bound_of(f):
    """blocks x blockMax: what lz4mt_hip.h asks of outCap and lz4mtHipStreamBound returns."""
    return len(f.recs) * F.block_max(f.params.bid)


def engine(frame, cap, stream=None):
    """lz4mtHipDecompressFrame into a tensor of ``cap`` bytes filled with a pattern:
    (result, bytes, whether the bytes past the decoded size still hold the pattern)."""
    src = dev(frame)
    out = torch.full((max(cap, 1),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()      # inputs ready before another stream reads them
    o, r = L.decompress_frame(src, out=out, stream=stream, check=False)
    return r, host(o), bool((out[o.numel():] == FILL).all().item())


def want_of(c, cap):
    """(code, bytes) of a case: the builder's; for a failing variant the oracle's as well."""
    want = C.expected(c)
    if c.fail is not None:
        assert oracle.decompress_frame(c.frame.frame, cap) == want, c.name
    return want


def check_engine(c, tag=""):
    f = c.frame
    cap = bound_of(f)
    if F.walk(f.frame) == len(f.recs):       # (a size word above blockMax ends the walk of the bound as well)
        assert L.stream_bound(dev(f.frame)) == cap, c.name
    r, got, tail = engine(f.frame, cap)
    code, text = want_of(c, cap)
    assert r == code, (c.name, tag, L.result_to_string(r))
    assert len(got) == len(text) and got == text, (c.name, tag, len(got), len(text), first_diff(got, text, f))
    return tail


def first_diff(got, text, f):
    """(position, block index) of the first differing byte, for the assertion message."""
    n = min(len(got), len(text))
    p = next((i for i in range(n) if got[i] != text[i]), n)
    return p, max(i for i, s in enumerate(f.starts) if s <= p) if f.starts else None


# ---------------------------------------------------------------------------
# linked frames on the device frame engine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.LINKED)
def test_linked_frames_device_engine(name):
    """Every linked frame and variant at the documented capacity; the engine decodes a linked
    frame in scratch of its own, so the tensor past the decoded size is untouched."""
    for c in C.cases(name):
        assert check_engine(c), c.name


@pytest.mark.parametrize("rounds", ["1", "2", "serial"])
@pytest.mark.parametrize("name", C.ROUNDS)
def test_linked_frames_round_caps(monkeypatch, name, rounds):
    """The parallel rounds capped at 1 and 2 (the serial finish gathers block after block over
    many short predecessors) and the one-wave kernel alone: same result, same bytes."""
    if rounds == "serial":
        monkeypatch.setenv("LZ4MT_AMD_BD_SERIAL", "1")
    else:
        monkeypatch.setenv("LZ4MT_AMD_BD_ROUNDS", rounds)
    for c in C.cases(name):
        assert check_engine(c, rounds), c.name


# ---------------------------------------------------------------------------
# linked frames through lz4mtDecompress
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("batches", ["default", "small"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", C.LINKED)
def test_linked_frames_callback_api(monkeypatch, name, mode, batches):
    """With 1 MiB batches a call decodes 16 blocks of 64 KiB block size: on "short", "many" and
    "chain" less than the window, so the history carried to the next batch is the old history's
    tail and the new bytes (k_dlink_hist_out below position 0, load_hist of k_decode_linked).
    The bytes delivered to the write callback before an error are the oracle's."""
    if batches == "small":
        monkeypatch.setenv("LZ4MT_AMD_BATCH0_MIB", "1")
        monkeypatch.setenv("LZ4MT_AMD_BATCH_MIB", "1")
    m = getattr(L, "MODE_" + mode)
    for c in C.cases(name):
        f = c.frame
        code, text = want_of(c, bound_of(f))
        r, got, sd = L.decompress(f.frame, len(f.text) + 64, mode=m)
        assert r == code, (c.name, mode, batches, L.result_to_string(r))
        assert len(got) == len(text) and got == text, (c.name, mode, batches, first_diff(got, text, f))
        assert sd.flg.blockIndependence == 0 and sd.bd.blockMaximumSize == f.params.bid


@pytest.mark.parametrize("rounds", ["1", "serial"])
@pytest.mark.parametrize("name", C.SHORT_BATCHES)
def test_short_batches_under_round_caps(monkeypatch, name, rounds):
    """The carried history of short batches with the serial finish and with the one-wave kernel
    (its load_hist reads the bytes before the call's output out of hist)."""
    monkeypatch.setenv("LZ4MT_AMD_BATCH0_MIB", "1")
    monkeypatch.setenv("LZ4MT_AMD_BATCH_MIB", "1")
    monkeypatch.setenv(*(("LZ4MT_AMD_BD_SERIAL", "1") if rounds == "serial" else ("LZ4MT_AMD_BD_ROUNDS", rounds)))
    for c in C.cases(name):
        code, text = want_of(c, bound_of(c.frame))
        r, got, _ = L.decompress(c.frame.frame, len(c.frame.text) + 64, mode=L.MODE_DEVICE)
        assert (r, len(got)) == (code, len(text)) and got == text, (c.name, rounds, first_diff(got, text, c.frame))


# ---------------------------------------------------------------------------
# frames of independent blocks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["serial", "parallel", "fused"])
@pytest.mark.parametrize("name", C.INDEP)
def test_independent_frames_device_engine(monkeypatch, name, walk):
    """k_decode behind the serial and the parallel walk, k_decode_walk: the builder's text, the
    oracle's code and bytes for the variant with an invalid block, and exactly the builder's
    record offsets."""
    monkeypatch.setenv("LZ4MT_AMD_WALK", walk)
    for c in C.cases(name):
        f = c.frame
        cap = bound_of(f)
        assert L.stream_bound(dev(f.frame)) == cap, c.name
        hl, recs, sd = L.frame_records(dev(f.frame))
        assert hl == 7 and recs == f.records, (c.name, walk)
        assert sd.flg.blockIndependence == 1 and sd.bd.blockMaximumSize == f.params.bid
        r, got, _ = engine(f.frame, cap)
        code, text = want_of(c, cap)
        assert r == code, (c.name, walk, L.result_to_string(r))
        assert len(got) == len(text) and got == text, (c.name, walk, first_diff(got, text, f))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", C.INDEP)
def test_independent_frames_callback_api(name, mode):
    """DEVICE mode is the streamed k_decode_stream; PARALLEL and SEQUENTIAL decode block by block."""
    m = getattr(L, "MODE_" + mode)
    for c in C.cases(name):
        f = c.frame
        code, text = want_of(c, bound_of(f))
        r, got, sd = L.decompress(f.frame, len(f.text) + 64, mode=m)
        assert r == code, (c.name, mode, L.result_to_string(r))
        assert len(got) == len(text) and got == text, (c.name, mode, first_diff(got, text, f))
        assert sd.flg.blockIndependence == 1


# ---------------------------------------------------------------------------
# damaged linked frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("api", ["device", "DEVICE"])
def test_damaged_short_frames_vs_oracle(api):
    """40 damaged copies of "short" (bit flips, truncations, rewritten words and size words; at
    least five still decode, at least five fail: asserted on the CPU): the oracle's result code
    and bytes, at one blockMax slot per record the damaged frame holds."""
    for k, d in enumerate(C.damaged_short()):
        cap = C.damaged_cap(d)
        rw, ow = oracle.decompress_frame(d, cap)
        if api == "device":
            r, got, _ = engine(d, cap)
        else:
            r, got, _ = L.decompress(d, cap, mode=L.MODE_DEVICE)
        assert r == rw, (k, L.result_to_string(r), L.result_to_string(rw))
        assert len(got) == len(ow) and got == ow, (k, len(got), len(ow))


# ---------------------------------------------------------------------------
# scratch reuse
# ---------------------------------------------------------------------------
def test_scratch_shrinks_and_grows_and_two_streams():
    """"short" (300 slots of 128 KiB), "b7" (24 of 4 MiB + 64 KiB), "short" again on one thread:
    the thread's scratch is cut anew for each slot stride.  Then two linked frames decoded in
    turn on two streams (the frame decode has no asynchronous form: each call returns after
    its own stream), each to its own text."""
    for label in ("short-SX", "b7-sx", "short-sx", "many-SX", "span-sx"):
        assert check_engine(C.case(label)), label
    a, b = C.case("chain-SX"), C.case("short-sx")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for c, st in [(a, streams[0]), (b, streams[1])] * 2:
        r, got, tail = engine(c.frame.frame, bound_of(c.frame), stream=st)
        assert r == 0 and got == c.frame.text and tail, c.name
    torch.cuda.synchronize()
