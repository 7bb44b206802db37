"""Batched block operators (lz4mtHipCompressBatch / lz4mtHipDecompressBatch)
on App. F synthetic input cut into uniform chunks of 4 KiB, 64 KiB and 1 MiB
and one ragged mix of 1 KiB .. 256 KiB, timed with device events (2 warm-up
calls discarded, median of 10), beside the frame engine's encode and decode
kernels on the same bytes at -B4 and -B6 (-Sx, no block checksum) as the
yardstick: the 64 KiB and 1 MiB batch kernels run the same window code on
the same blocks.  Prints one JSON line.

    python tools/batch_bench.py [--gib 1] [--reps 10] [--level L] [--dict-kib K] [--dicts N] [--rows 4KiB,64KiB]

--level L times lz4mtHipCompressBatchEx at that level instead (L >= 3:
LZ4-HC, its workspace of the full lz4mtHipCompressBatchWorkspaceSize unless
--slots caps it) beside the frame engine's encode time at the same level,
which is then the chain and parse kernels together, as the batch call's is.
At 1 MiB the frame engine splits each block's parse over several waves and
the batch does not: that row is a ratio to record, not a yardstick.

--dict-kib K times the dictionary calls (lz4mtHipCompressBatchDict /
lz4mtHipDecompressBatchDict; lz4mtHipDictPrepare on its own) with a
dictionary of K KiB, the last K KiB of the same App. F input in a tensor of
its own.  The yardstick is then the plain batch call on the same chunks in
the same run: every row carries both times, both compression ratios and
their quotients, and the frame rows are left out.

--level L with --dict-kib K (L >= 3) times lz4mtHipCompressBatchDictHC
(lz4mtHipDictPrepareHC on its own).  Two yardsticks in every row: the plain
lz4mtHipCompressBatchEx call at the same level on the same chunks for the
time ("plain_*"), and the fast dictionary call lz4mtHipCompressBatchDict with
the same dictionary for the ratio ("fast_dict_*").

--dicts N with --dict-kib K (the fast codec) also times the calls with a
set of dictionaries (lz4mtHipCompressBatchDictSet /
lz4mtHipDecompressBatchDictSet; lz4mtHipDictSetPrepare on its own): N
dictionaries of K KiB, chunk i using dictionary i % N.  The N dictionaries
hold the same bytes in N allocations of their own, and so do their N states:
the set calls then do the shared-dictionary call's work on the same chunks
(the sizes are compared) and differ from it in the per-chunk loads and in the
memory the tables and dictionaries are read from.  The yardstick is the
shared-dictionary call in the same row ("set_*_over_shared").

--dicts N with --dict-kib K and --level L >= 3 times the LZ4-HC set call
(lz4mtHipCompressBatchDictSetHC; lz4mtHipDictSetPrepareHC on its own) on the
same layout: N allocations of the same K KiB, N states, chunk i using
dictionary i % N.  Two yardsticks on the same chunks in the same run: the
shared-dictionary call lz4mtHipCompressBatchDictHC ("set_compress_over_shared")
and N calls of it, one per dictionary over that dictionary's chunks, what a
caller without the set call has to issue ("separate_*",
"set_compress_over_separate").  The sizes of both are compared with the shared
call's.

--rows picks the chunkings to run (4KiB, 64KiB, 1MiB, ragged; default all).

Capacities are the default (d_dstCaps = NULL: the bound of each size), the
frame encoder's are the block size; every configuration is decoded back and
compared with the input once, outside the timed calls.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lz4mt_amd as L  # noqa: E402

P = ctypes.c_void_p


def timed(fn, reps, warm=2):
    """median, min, max (ms, device events) of `reps` calls after `warm` discarded ones"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def batch_row(name, src, sizes, reps, level=0, slots=0, dct=None):
    n = len(sizes)
    total = int(sizes.sum())
    soff = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    caps = sizes + sizes // 255 + 16
    stride = (caps + 15) & ~np.int64(15)
    doff = np.concatenate([[0], np.cumsum(stride)[:-1]]).astype(np.int64)
    comp = torch.empty(int(stride.sum()), dtype=torch.uint8, device="cuda")
    back = torch.empty(int(((sizes + 15) & ~np.int64(15)).sum()), dtype=torch.uint8, device="cuda")
    boff = np.concatenate([[0], np.cumsum((sizes + 15) & ~np.int64(15))[:-1]]).astype(np.int64)
    sp = torch.from_numpy(soff + src.data_ptr()).cuda()
    cp = torch.from_numpy(doff + comp.data_ptr()).cuda()
    bp = torch.from_numpy(boff + back.data_ptr()).cuda()
    sz = torch.from_numpy(sizes.astype(np.uint32).view(np.int32)).cuda()
    csz = torch.zeros(n, dtype=torch.int32, device="cuda")
    dsz = torch.zeros(n, dtype=torch.int32, device="cuda")
    max_chunk = int(sizes.max())
    st = P(torch.cuda.current_stream().cuda_stream)

    ws = None
    if level >= 3:
        ws = L.batch_compress_workspace(max_chunk, min(n, slots) if slots else n, level)
    nslots = ws.numel() // L.lib.lz4mtHipCompressBatchWorkspaceSize(max_chunk, 1, level) if level >= 3 else 0

    def enc():
        if level == 0:
            r = L.lib.lz4mtHipCompressBatch(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, n, P(cp.data_ptr()), None,
                                            P(csz.data_ptr()), st)
        else:
            r = L.lib.lz4mtHipCompressBatchEx(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, n, P(cp.data_ptr()), None,
                                              P(csz.data_ptr()), level, P(ws.data_ptr() if level >= 3 else None),
                                              ws.numel() if level >= 3 else 0, st)
        assert r == 0, r

    def dec():
        r = L.lib.lz4mtHipDecompressBatch(P(cp.data_ptr()), P(csz.data_ptr()), n, P(bp.data_ptr()), P(sz.data_ptr()),
                                          P(dsz.data_ptr()), st)
        assert r == 0, r

    def round_trip():   # once per codec: sizes and bytes
        assert bool((csz > 0).all()) and torch.equal(dsz, sz), name
        if bool(np.all(boff[1:] - boff[:-1] == sizes[:-1])):   # outputs contiguous: one compare
            assert torch.equal(back[:total], src[:total]), name
        else:
            for i in np.random.RandomState(1).choice(n, size=min(n, 2000), replace=False):
                a, b, k = int(boff[i]), int(soff[i]), int(sizes[i])
                assert torch.equal(back[a:a + k], src[b:b + k]), (name, int(i))

    e = timed(enc, reps)
    d = timed(dec, reps)
    round_trip()
    cbytes = int(csz.sum().item())
    gib = total / 2**30
    if dct is not None:
        dictionary, state, state_hc, dset = dct

        def enc_f():
            r = L.lib.lz4mtHipCompressBatchDict(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, n, P(cp.data_ptr()),
                                                None, P(csz.data_ptr()), P(dictionary.data_ptr()), dictionary.numel(),
                                                P(state.data_ptr()), st)
            assert r == 0, r

        def enc_hc():
            r = L.lib.lz4mtHipCompressBatchDictHC(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, n, P(cp.data_ptr()),
                                                  None, P(csz.data_ptr()), P(dictionary.data_ptr()),
                                                  dictionary.numel(), P(state_hc.data_ptr()), level,
                                                  P(ws.data_ptr()), ws.numel(), st)
            assert r == 0, r

        enc_d = enc_hc if level >= 3 else enc_f
        fast = {}
        if level >= 3:   # the ratio's yardstick: the fast codec with the same dictionary
            ef = timed(enc_f, reps)
            fast = {"fast_dict_ratio": round(total / int(csz.sum().item()), 4), "fast_dict_compress_ms": round(ef[0], 3),
                    "fast_dict_compress_ms_min_max": [round(ef[1], 3), round(ef[2], 3)]}

        def dec_d():
            r = L.lib.lz4mtHipDecompressBatchDict(P(cp.data_ptr()), P(csz.data_ptr()), n, P(bp.data_ptr()),
                                                  P(sz.data_ptr()), P(dsz.data_ptr()), P(dictionary.data_ptr()),
                                                  dictionary.numel(), st)
            assert r == 0, r

        back.zero_()
        ed = timed(enc_d, reps)
        dd = timed(dec_d, reps)
        round_trip()
        dbytes = int(csz.sum().item())
        sset = {}
        if dset is not None:   # the same chunks through the set calls, chunk i with dictionary i % N
            d_ptrs, d_sizes, states, nd, copies = dset
            which = torch.from_numpy((np.arange(n, dtype=np.int64) % nd).astype(np.int32)).cuda()
            shared_sizes = csz.clone()

            def enc_s():
                r = L.lib.lz4mtHipCompressBatchDictSet(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, n,
                                                       P(cp.data_ptr()), None, P(csz.data_ptr()), P(d_ptrs.data_ptr()),
                                                       P(d_sizes.data_ptr()), nd, P(states.data_ptr()),
                                                       P(which.data_ptr()), st)
                assert r == 0, r

            def dec_s():
                r = L.lib.lz4mtHipDecompressBatchDictSet(P(cp.data_ptr()), P(csz.data_ptr()), n, P(bp.data_ptr()),
                                                         P(sz.data_ptr()), P(dsz.data_ptr()), P(d_ptrs.data_ptr()),
                                                         P(d_sizes.data_ptr()), nd, P(which.data_ptr()), st)
                assert r == 0, r

            if level >= 3:
                sset = hc_set_part(name, reps, level, n, max_chunk, nd, copies, d_ptrs, d_sizes, states, which, ws, st,
                                   sp, sz, cp, csz, soff + src.data_ptr(), doff + comp.data_ptr(), sizes,
                                   shared_sizes, ed)
                back.zero_()
                timed(dec_s, 1, warm=0)   # the set call's blocks through the set decoder, once
                round_trip()
            else:
                csz.zero_()
                back.zero_()
                es = timed(enc_s, reps)
                dz = timed(dec_s, reps)
                assert torch.equal(csz, shared_sizes), name   # the same dictionary bytes: the same blocks
                round_trip()
                sset = {"dicts": nd, "set_kernel": "k_encode_batch_dict<DictSet> / k_decode_batch_dict_set",
                        "set_compress_ms": round(es[0], 3),
                        "set_compress_ms_min_max": [round(es[1], 3), round(es[2], 3)],
                        "set_decompress_ms": round(dz[0], 3),
                        "set_decompress_ms_min_max": [round(dz[1], 3), round(dz[2], 3)],
                        "set_compress_over_shared": round(es[0] / ed[0], 4),
                        "set_decompress_over_shared": round(dz[0] / dd[0], 4)}
        kernel, plain = "k_encode_batch_dict<SharedDict>", "k_encode_batch16" if max_chunk < 65547 else "k_encode_batch"
        if level >= 3:
            parse = "k_encode_hc_opt_batch" if level >= 10 else "k_encode_hc_batch"
            kernel = f"k_hc_prev_batch<HcSharedDict> + {parse}<HcSharedDict>"
            plain = f"k_hc_prev_batch<HcNoDict> + {parse}<HcNoDict>"
            fast.update({"slots": nslots, "rounds": -(-n // nslots), "workspace_bytes": ws.numel()})
        return {"name": name, "chunks": n, "bytes": total, "max_chunk": max_chunk,
                "kernel": kernel + " / k_decode_batch_dict", "plain_kernel": plain, **fast, **sset,
                "ratio": round(total / dbytes, 4), "plain_ratio": round(total / cbytes, 4),
                "compress_ms": round(ed[0], 3), "compress_ms_min_max": [round(ed[1], 3), round(ed[2], 3)],
                "compress_gib_s": round(gib / (ed[0] / 1e3), 2),
                "decompress_ms": round(dd[0], 3), "decompress_ms_min_max": [round(dd[1], 3), round(dd[2], 3)],
                "decompress_gib_s": round(gib / (dd[0] / 1e3), 2),
                "plain_compress_ms": round(e[0], 3), "plain_compress_ms_min_max": [round(e[1], 3), round(e[2], 3)],
                "plain_decompress_ms": round(d[0], 3),
                "plain_decompress_ms_min_max": [round(d[1], 3), round(d[2], 3)],
                "compress_over_plain": round(ed[0] / e[0], 4), "decompress_over_plain": round(dd[0] / d[0], 4)}
    kernel = "k_encode_batch16" if max_chunk < 65547 else "k_encode_batch"
    if level >= 3:
        kernel = "k_hc_prev_batch + " + ("k_encode_hc_opt_batch" if level >= 10 else "k_encode_hc_batch")
    hc = {"slots": nslots, "rounds": -(-n // nslots), "workspace_bytes": ws.numel()} if level >= 3 else {}
    return {"name": name, "chunks": n, "bytes": total, "max_chunk": max_chunk, **hc,
            "kernel": kernel, "ratio": round(total / cbytes, 4),
            "compress_ms": round(e[0], 3), "compress_ms_min_max": [round(e[1], 3), round(e[2], 3)],
            "compress_gib_s": round(gib / (e[0] / 1e3), 2),
            "decompress_ms": round(d[0], 3), "decompress_ms_min_max": [round(d[1], 3), round(d[2], 3)],
            "decompress_gib_s": round(gib / (d[0] / 1e3), 2)}


def hc_set_part(name, reps, level, n, max_chunk, nd, copies, d_ptrs, d_sizes, states, which, ws, st, sp, sz, cp, csz,
                src_ptrs, dst_ptrs, sizes, shared_sizes, ed):
    """lz4mtHipCompressBatchDictSetHC, and nd calls of lz4mtHipCompressBatchDictHC over each dictionary's
    chunks (the arrays permuted so that a dictionary's chunks stand together), against the shared call ``ed``."""
    S = L.lib.lz4mtHipDictStateSizeHC()

    def enc_s():
        r = L.lib.lz4mtHipCompressBatchDictSetHC(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, n, P(cp.data_ptr()),
                                                 None, P(csz.data_ptr()), P(d_ptrs.data_ptr()), P(d_sizes.data_ptr()),
                                                 nd, P(states.data_ptr()), P(which.data_ptr()), level,
                                                 P(ws.data_ptr()), ws.numel(), st)
        assert r == 0, r

    own = np.arange(n, dtype=np.int64) % nd
    perm = np.argsort(own, kind="stable")
    counts = np.bincount(own, minlength=nd)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    sp_p = torch.from_numpy(src_ptrs[perm]).cuda()
    cp_p = torch.from_numpy(dst_ptrs[perm]).cuda()
    sz_p = torch.from_numpy(sizes[perm].astype(np.uint32).view(np.int32)).cuda()
    csz_p = torch.zeros(n, dtype=torch.int32, device="cuda")

    def enc_k():
        for j in range(nd):
            o, g = int(starts[j]), int(counts[j])
            if g == 0:
                continue
            r = L.lib.lz4mtHipCompressBatchDictHC(P(sp_p.data_ptr() + 8 * o), P(sz_p.data_ptr() + 4 * o), max_chunk, g,
                                                  P(cp_p.data_ptr() + 8 * o), None, P(csz_p.data_ptr() + 4 * o),
                                                  P(copies[j].data_ptr()), copies[j].numel(),
                                                  P(states.data_ptr() + j * S), level, P(ws.data_ptr()), ws.numel(),
                                                  st)
            assert r == 0, r

    ek = timed(enc_k, reps)
    assert torch.equal(csz_p, shared_sizes[torch.from_numpy(perm).cuda()]), name
    csz.zero_()
    es = timed(enc_s, reps)
    assert torch.equal(csz, shared_sizes), name   # the same dictionary bytes: the same blocks
    return {"dicts": nd,
            "set_kernel": "k_hc_prev_batch<HcDictSet> + " + ("k_encode_hc_opt_batch" if level >= 10 else
                                                            "k_encode_hc_batch") + "<HcDictSet>",
            "set_compress_ms": round(es[0], 3), "set_compress_ms_min_max": [round(es[1], 3), round(es[2], 3)],
            "separate_calls": int((counts > 0).sum()),
            "separate_compress_ms": round(ek[0], 3),
            "separate_compress_ms_min_max": [round(ek[1], 3), round(ek[2], 3)],
            "set_compress_over_shared": round(es[0] / ed[0], 4),
            "set_compress_over_separate": round(es[0] / ek[0], 4)}


def frame_row(src, bid, reps, level=0):
    """the frame engine's encode kernel (timing slot 0 of the compress call) and
    decode kernel (slot 1 of the decompress call), as tools/ktime.py reads them"""
    sd = L.make_sd(bid, False, False)
    ws = L.compress_workspace(src.numel(), sd, level=level)
    out = torch.empty(L.frame_bound(src.numel(), sd), dtype=torch.uint8, device="cuda")
    dst = torch.empty(src.numel() + (4 << 20), dtype=torch.uint8, device="cuda")
    ms = (ctypes.c_float * 4)()
    L.lib.lz4mtHipSetTiming(1)
    enc, dec = [], []
    for i in range(reps + 2):
        fr = L.compress_frame(src, sd, out=out, workspace=ws, level=level)
        assert L.lib.lz4mtHipGetTimings(ms) == 0
        e = ms[0]
        got, r = L.decompress_frame(fr, out=dst)
        assert r == 0 and L.lib.lz4mtHipGetTimings(ms) == 0
        if i >= 2:
            enc.append(e)
            dec.append(ms[1])
    L.lib.lz4mtHipSetTiming(0)
    assert torch.equal(got, src)
    gib = src.numel() / 2**30
    e, d = statistics.median(enc), statistics.median(dec)
    return {"name": f"frame -B{bid} -Sx", "block": 1 << (8 + 2 * bid), "encode_kernel_ms": round(e, 3),
            "encode_kernel_ms_min_max": [round(min(enc), 3), round(max(enc), 3)],
            "encode_gib_s": round(gib / (e / 1e3), 2), "decode_kernel_ms": round(d, 3),
            "decode_kernel_ms_min_max": [round(min(dec), 3), round(max(dec), 3)],
            "decode_gib_s": round(gib / (d / 1e3), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--level", type=int, default=0, help="compression level of the batch and the frame calls")
    ap.add_argument("--slots", type=int, default=0, help="level >= 3: cap the workspace at this many slots")
    ap.add_argument("--dict-kib", type=int, default=0, help="time the dictionary calls with a dictionary of K KiB")
    ap.add_argument("--dicts", type=int, default=0,
                    help="with --dict-kib: also time the set calls with N dictionaries, chunk i using i %% N")
    ap.add_argument("--rows", default="4KiB,64KiB,1MiB,ragged", help="chunkings to run")
    a = ap.parse_args()
    want = set(a.rows.split(","))
    if not want <= {"4KiB", "64KiB", "1MiB", "ragged"}:
        sys.exit("--rows: a comma-separated subset of 4KiB,64KiB,1MiB,ragged")
    if a.dicts and (not a.dict_kib or a.dicts < 0):
        sys.exit("--dicts: a count of dictionaries, with --dict-kib")
    if not torch.cuda.is_available():
        sys.exit("batch_bench.py needs a HIP device")
    n = int(a.gib * 2**30) & ~((1 << 20) - 1)
    src = L.gen_synthetic(n, seed=42)
    dct, prep = None, {}
    if a.dict_kib:
        dictionary = src[n - (a.dict_kib << 10):].clone()
        state = torch.empty(L.lib.lz4mtHipDictStateSize(), dtype=torch.uint8, device="cuda")
        st = P(torch.cuda.current_stream().cuda_stream)

        def prepare():
            r = L.lib.lz4mtHipDictPrepare(P(dictionary.data_ptr()), dictionary.numel(), P(state.data_ptr()),
                                          state.numel(), st)
            assert r == 0, r

        pm = timed(prepare, a.reps)
        state_hc = None
        prep = {"dict_bytes": dictionary.numel(), "dict": "the input's last bytes", "state_bytes": state.numel(),
                "prepare_ms": round(pm[0], 4), "prepare_ms_min_max": [round(pm[1], 4), round(pm[2], 4)]}
        if a.level >= 3:
            state_hc = torch.empty(L.lib.lz4mtHipDictStateSizeHC(), dtype=torch.uint8, device="cuda")

            def prepare_hc():
                r = L.lib.lz4mtHipDictPrepareHC(P(dictionary.data_ptr()), dictionary.numel(), P(state_hc.data_ptr()),
                                                state_hc.numel(), st)
                assert r == 0, r

            ph = timed(prepare_hc, a.reps)
            prep.update({"fast_state_bytes": state.numel(), "fast_prepare_ms": prep["prepare_ms"],
                         "state_bytes": state_hc.numel(), "prepare_ms": round(ph[0], 4),
                         "prepare_ms_min_max": [round(ph[1], 4), round(ph[2], 4)]})
        dset = None
        if a.dicts:   # N allocations of the same bytes (alive until main returns), N states
            copies = [dictionary.clone() for _ in range(a.dicts)]
            d_ptrs = torch.tensor([c.data_ptr() for c in copies], dtype=torch.int64, device="cuda")
            d_sizes = torch.tensor([c.numel() for c in copies], dtype=torch.int32, device="cuda")
            one = state_hc if a.level >= 3 else state
            set_prepare = L.lib.lz4mtHipDictSetPrepareHC if a.level >= 3 else L.lib.lz4mtHipDictSetPrepare
            states = torch.empty(a.dicts * one.numel(), dtype=torch.uint8, device="cuda")

            def prepare_set():
                r = set_prepare(P(d_ptrs.data_ptr()), P(d_sizes.data_ptr()), a.dicts, P(states.data_ptr()),
                                states.numel(), st)
                assert r == 0, r

            ps = timed(prepare_set, a.reps)
            assert torch.equal(states.view(a.dicts, -1), one.view(1, -1).expand(a.dicts, -1))
            prep.update({"dicts": a.dicts, "set_states_bytes": states.numel(),
                         "set_prepare_ms": round(ps[0], 4), "set_prepare_ms_min_max": [round(ps[1], 4), round(ps[2], 4)]})
            dset = (d_ptrs, d_sizes, states, a.dicts, copies)
        dct = (dictionary, state, state_hc, dset)
    rows = []
    for name, k in (("4KiB", 4 << 10), ("64KiB", 64 << 10), ("1MiB", 1 << 20)):
        if name in want:
            rows.append(batch_row(name, src, np.full(n // k, k, dtype=np.int64), a.reps, a.level, a.slots, dct))
    rs = np.random.RandomState(7)
    sizes = rs.randint(1 << 10, (256 << 10) + 1, size=2 * n // (128 << 10) + 16).astype(np.int64)
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), n, side="right"))]
    if "ragged" in want:
        rows.append(batch_row("ragged 1KiB-256KiB", src, sizes, a.reps, a.level, a.slots, dct))
    if dct is not None:   # the yardstick is the plain batch call, in every row
        print(json.dumps({"tool": "batch_bench", "device": torch.cuda.get_device_name(0),
                          "input": "gen_synthetic seed 42", "bytes": n, "level": a.level if a.level >= 3 else 0,
                          "reps": a.reps, "warmup": 2, "stat": "median", **prep, "batch": rows}))
        return
    if not {"64KiB", "1MiB"} <= want:
        sys.exit("the frame yardstick needs the 64KiB and 1MiB rows")
    frames = [frame_row(src, 4, a.reps, a.level), frame_row(src, 6, a.reps, a.level)]
    by = {r["name"]: r for r in rows}
    gaps = {}
    for nm, fr in (("64KiB", frames[0]), ("1MiB", frames[1])):
        gaps[nm] = {"encode_vs_frame_kernel": round(by[nm]["compress_ms"] / fr["encode_kernel_ms"], 4),
                    "decode_vs_frame_kernel": round(by[nm]["decompress_ms"] / fr["decode_kernel_ms"], 4)}
    print(json.dumps({"tool": "batch_bench", "device": torch.cuda.get_device_name(0), "input": "gen_synthetic seed 42",
                      "bytes": n, "level": a.level, "reps": a.reps, "warmup": 2, "stat": "median", "batch": rows, "frame": frames,
                      "batch_over_frame_kernel": gaps}))


if __name__ == "__main__":
    main()
