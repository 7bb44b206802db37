"""An LZ4 frame builder over the block synthesizer (lz4_synth.py).

``FrameBuilder`` collects records -- synthesized or hand-written compressed
blocks, stored blocks, records that are wrong on purpose -- and ``frame``
writes them as an LZ4 frame: magic, FLG, BD, the header check byte, per block
the size word (bit 31 = stored), the payload and an optional XXH32, the EOS
word and an optional content XXH32.  Block ids 4..7, blocks independent or
linked.

In a linked frame the block at text position P is synthesized against the
last 65 536 bytes of ``bytes(65536) + text[:P]``: LZ4_decompress_safe_withPrefix64k
over the reference's zero-filled buffer (decompressBlockDependency).  Every
16-bit offset is then in range, and the synthesizer's byte-by-byte text is
the expected output with no decoder behind it.  ``lz4f=True`` hands over only
``text[:P][-65536:]``, so no sequence reaches before the frame's first byte
(liblz4's LZ4F_decompress rejects such offsets; lz4mt reads zeros).

The builder classifies every match of a linked frame by where its source
lies in the frame (``stats``, and per block ``block_stats``):
  ("blocks", "compressed" | "stored" | "zero")   records by kind; "zero": decoded size 0
  ("back", 0 | 1 | 2 | "3..9" | "10+")            blocks back to the block the source starts in
  "span2"       the source's bytes before the block lie in two or more earlier blocks
  "stored_src"  some of them lie in a stored block
  "prestart"    the source begins before the frame's first byte
  "hist_to_own" the source begins before the block and runs into the block's own output
The per-sequence counts of lz4_synth are summed into ``stats`` as well.

Pure Python; nothing here needs a GPU or a decoder.
"""
import bisect
import collections
import struct

import xxhash

import lz4_synth as S

MAGIC = 0x184D2204
RAW_BIT = 0x80000000
WINDOW = 65536

Rec = collections.namedtuple("Rec", "payload stored size_word checksum")
Frame = collections.namedtuple("Frame", "frame text records sizes starts stats block_stats recs params")
Params = collections.namedtuple("Params", "bid linked block_checksum content_checksum")


def block_max(bid):
    return 1 << (8 + 2 * bid)


def xxh32(b):
    return xxhash.xxh32(bytes(b), seed=0).intdigest()


def header(p):
    flg = 0x40 | (0 if p.linked else 0x20) | (0x10 if p.block_checksum else 0) | (0x04 if p.content_checksum else 0)
    desc = bytes([flg, p.bid << 4])
    return struct.pack("<I", MAGIC) + desc + bytes([(xxh32(desc) >> 8) & 0xFF])


def rec(payload, stored=False, size_word=None, checksum=None):
    """A record; ``size_word`` / ``checksum`` override what the payload implies."""
    return Rec(bytes(payload), stored, size_word, checksum)


def assemble(p, recs, text):
    """(frame bytes, [offset of every record's size word..., offset of the EOS word])."""
    out = bytearray(header(p))
    offs = []
    for r in recs:
        offs.append(len(out))
        word = r.size_word if r.size_word is not None else len(r.payload) | (RAW_BIT if r.stored else 0)
        out += struct.pack("<I", word) + r.payload
        if p.block_checksum:
            out += struct.pack("<I", r.checksum if r.checksum is not None else xxh32(r.payload))
    offs.append(len(out))
    out += bytes(4)
    if p.content_checksum:
        out += struct.pack("<I", xxh32(text))
    return bytes(out), offs


def back_class(k):
    return k if k <= 2 else "3..9" if k <= 9 else "10+"


class FrameBuilder:
    def __init__(self, bid=4, linked=True, lz4f=False):
        assert 4 <= bid <= 7
        self.bid, self.linked, self.lz4f = bid, linked, lz4f
        self.bm = block_max(bid)
        self.text = bytearray()
        self.recs, self.sizes, self.starts = [], [], []
        self.stats = collections.Counter()
        self.block_stats = []
        self.sources = []       # (block index, text position of the source, length) of every match of a linked frame

    # -- what the next block sees -------------------------------------------
    @property
    def n(self):
        return len(self.recs)

    def hist(self):
        """The dictionary of the next block (empty in a frame of independent blocks)."""
        if not self.linked:
            return b""
        tail = bytes(self.text[-WINDOW:])
        return tail if self.lz4f else bytes(WINDOW - len(tail)) + tail

    def writer(self, rnd):
        return S.Writer(rnd, self.hist())

    # -- records ------------------------------------------------------------
    def _append(self, r, plain, kind, matches=()):
        bs = collections.Counter()
        bs[("blocks", kind)] += 1
        if len(plain) == 0:
            bs[("blocks", "zero")] += 1
        T, i = len(self.text), self.n
        if self.linked:
            for P, off, mlen in matches:
                self.sources.append((i, T + P - off, mlen))
                self._classify(bs, i, T, T + P - off, mlen)
        self.recs.append(r)
        self.starts.append(T)
        self.sizes.append(len(plain))
        self.text += plain
        self.block_stats.append(bs)
        self.stats.update(bs)
        return i

    def _block_of(self, g):
        """The block that holds text position g >= 0 (among the blocks added so far)."""
        return bisect.bisect_right(self.starts, g) - 1

    def _classify(self, bs, i, T, G, mlen):
        if G >= T:
            bs[("back", 0)] += 1
            return
        if G + mlen > T:
            bs["hist_to_own"] += 1
        if G < 0:
            bs["prestart"] += 1
        first = self._block_of(max(G, 0)) if max(G, 0) < T else i
        last = self._block_of(min(G + mlen, T) - 1) if min(G + mlen, T) > 0 else -1
        if G >= 0:
            bs[("back", back_class(i - first))] += 1
        if last >= 0:
            held = [k for k in range(first, last + 1) if self.sizes[k]]
            if len(held) >= 2:
                bs["span2"] += 1
            if any(self.recs[k].stored for k in held):
                bs["stored_src"] += 1

    def add_block(self, block, plain, matches=(), stats=None):
        """A compressed block with its plain text (from a Writer or S.synth)."""
        if stats:
            self.stats.update(stats)
        return self._append(rec(block), plain, "compressed", matches)

    def add_writer(self, w, lit=None):
        block, plain, stats = w.finish(lit)
        assert w.valid
        return self.add_block(block, plain, w.matches, stats)

    def add_synth(self, rnd, n_target, profile="mixed"):
        ws = []
        block, plain, stats = S.synth(rnd, self.hist(), n_target, profile, writer=ws)
        return self.add_block(block, plain, ws[0].matches, stats)

    def add_stored(self, data):
        return self._append(rec(data, stored=True), bytes(data), "stored")

    def add_directed(self, rnd, backs, span=False):
        """A block with one match per entry of ``backs`` whose source starts that many blocks
        back (in a block that decodes to something); ``span``: long enough to run over the
        following block's end as well, where two earlier blocks follow the source."""
        w = self.writer(rnd)
        T, i = len(self.text), self.n
        for k in backs:
            j = i - k
            if j < 0 or not self.sizes[j]:
                continue
            G = self.starts[j] + rnd.randrange(self.sizes[j])
            lit = rnd.randrange(0, 6)
            off = T + w.op + lit - G
            if off > S.MAX_OFF:
                continue
            mlen = rnd.randrange(4, 24)
            if span:
                mlen = max(mlen, min(self.starts[j] + self.sizes[j] - G + rnd.randrange(4, 300), 5000))
            w.seq(lit, off, mlen)
        return self.add_writer(w)

    # -- the frame ----------------------------------------------------------
    def frame(self, block_checksum, content_checksum, recs=None):
        """The Frame of the records added (``recs``: another record list over the same text, for
        the variants that fail)."""
        p = Params(self.bid, self.linked, block_checksum, content_checksum)
        recs = list(self.recs) if recs is None else recs
        data, offs = assemble(p, recs, self.text)
        return Frame(data, bytes(self.text), offs, list(self.sizes), list(self.starts), self.stats,
                     self.block_stats, recs, p)


def text_before(f, i):
    """The concatenated text of the blocks before block i, from the builder's sizes."""
    return f.text[:sum(f.sizes[:i])]


def contract_cap(f):
    """The output capacity of the decoders' contract: one blockMax slot per record (and the
    stored lengths on top, which the oracle counts exactly)."""
    return len(f.recs) * block_max(f.params.bid) + sum(len(r.payload) for r in f.recs if r.stored)


def walk(frame):
    """The number of records a reader finds before the EOS word, a size word above blockMax or
    the end of the bytes (damaged frames: how many slots the contract's capacity has to hold)."""
    if len(frame) < 7:
        return 0
    flg, bd = frame[4], frame[5]
    bm = block_max((bd >> 4) & 7) if 4 <= (bd >> 4) & 7 <= 7 else 0
    pos = 7 + (8 if flg & 0x08 else 0)
    n = 0
    while pos + 4 <= len(frame):
        word = struct.unpack_from("<I", frame, pos)[0]
        size = word & 0x7FFFFFFF
        if word == 0 or size > bm:
            break
        pos += 4 + size + (4 if flg & 0x10 else 0)
        n += 1
    return n


def damaged_frames(rnd, frame, count, records):
    """Bit flips, truncations and rewritten words, drawn as test_gpu_bd.py draws them; every
    other rewritten word is a record's size word (``records``: their offsets), changed by a
    little or in its stored bit, so that the frame walk goes on from a wrong place."""
    out = []
    for it in range(count):
        b = bytearray(frame)
        kind = it % 3
        if kind == 0:
            b[rnd.randrange(7, len(b))] ^= 1 << rnd.randrange(8)
        elif kind == 1:
            del b[rnd.randrange(8, len(b)):]
        elif it % 2:
            a = records[rnd.randrange(len(records) - 1)]
            word = int.from_bytes(b[a:a + 4], "little")
            word = word ^ RAW_BIT if rnd.random() < 0.3 else max(word + rnd.choice((-9, -4, -1, 1, 2, 5, 300)), 1)
            b[a:a + 4] = word.to_bytes(4, "little")
        else:
            a = rnd.randrange(7, len(b) - 4)
            b[a:a + 4] = rnd.randrange(1 << 32).to_bytes(4, "little")
        out.append(bytes(b))
    return out
