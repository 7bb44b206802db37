"""Compares tools/lz4hc_dict_model.c (the host restatement of LZ4-HC 1.9.3 with
an external dictionary that the HcDictBlock kernels were ported from) with
liblz4 1.9.3: every case of the two fixtures' plans (tests/dict_hc_cases.py)
and --random further seeded cases.  CPU only.

usage: python tools/lz4hc_dict_diff.py [--random N] [--seed S] [--skip-plan]
"""
import argparse
import ctypes
import importlib.util
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dict_hc_cases as H  # noqa: E402


def load_model(tmp):
    so = os.path.join(tmp, "hcdict_model.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "lz4hc_dict_model.c")])
    lib = ctypes.CDLL(so)
    lib.hcdict_model_compress.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32,
                                          ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int]
    return lib


def model(lib, d, src, cap, level):
    ob = ctypes.create_string_buffer(cap + 64)
    n = lib.hcdict_model_compress(bytes(d), len(d), bytes(src), len(src), ob, cap, level)
    return ob.raw[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--random", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--skip-plan", action="store_true")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("gen", os.path.join(ROOT, "tests", "golden", "make_golden_dict_hc.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    lz = gen.load_lz4()
    bad = total = 0
    with tempfile.TemporaryDirectory() as tmp:
        lib = load_model(tmp)

        def check(tag, d, src, cap, level):
            nonlocal bad, total
            total += 1
            want, got = gen.compress(lz, d, src, cap, level), model(lib, d, src, cap, level)
            if want != got:
                bad += 1
                if bad <= 20:
                    print("DIFF", tag, "dict", len(d), "n", len(src), "cap", cap, "level", level, "liblz4", len(want),
                          "model", len(got))

        if not a.skip_plan:
            for dspec, items in H.plan():
                d = H.make_dict(dspec)
                for name, level, capkind in items:
                    src = H.make_chunk(name, d, dspec["seed"])
                    check((dspec, name), d, src, H.cap_of(capkind, len(src)), level)
            dicts = [H.make_dict(s) for s in H.FUZZ_DICTS]
            for di, kind, n, seed, level, capkind in H.fuzz_plan():
                check(("fuzz", di, kind, seed), dicts[di], H.fuzz_chunk(kind, n, seed, dicts[di]), H.cap_of(capkind, n), level)
            print(f"plans: {total} cases, {bad} differ")
        rnd = random.Random(a.seed)
        for i in range(a.random):
            spec_ = H.dict_spec(rnd.choice([0, 1, 3, 4, 7, 64, 1000, 4096, 30000, 65535, 65536, 66000]),
                                seed=rnd.randrange(20, 24), run=rnd.choice([0, 0, 1, 2, 3, 4, 5, 9, 60]))
            if spec_["run"] > spec_["size"]:
                spec_["run"] = 0
            d = H.make_dict(spec_)
            n = rnd.choice([rnd.randrange(0, 40), rnd.randrange(40, 3000), rnd.randrange(3000, 20000)])
            if rnd.random() < 0.03:
                n = rnd.randrange(60000, 140000)
            kind, seed = rnd.choice(H.FUZZ_KINDS), rnd.randrange(1 << 30)
            check((spec_, kind, seed), d, H.fuzz_chunk(kind, n, seed, d), H.cap_of(rnd.choice(H.CAP_KINDS), n),
                  rnd.randrange(3, 14))
        print(f"total: {total} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
