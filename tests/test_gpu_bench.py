"""bench.py's single-GPU entry: a plain run times the steps and prints the
line (no CPU baseline), --full adds the baseline, --dump-outputs writes the
last step's frame and decoded bytes so two builds can be compared array for
array (same arguments: same seeded input, same arrays)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import xxhash

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 28   # --gib 0.25


def _bench(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--gib", "0.25", *args],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    lines = [_bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 2 and line["warmup"] == 1 and line["roundtrip_ok"] is True
        assert line["ms_per_step"] > 0 and line["unit"] == "GiB/s" and line["higher_is_better"] is True
        # value = GiB per second of one step's compress + decompress
        assert line["value"] == pytest.approx(N / (1 << 30) / (line["ms_per_step"] * 1e-3), rel=1e-3)
        assert line["cpu_baseline"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert names == sorted(f"{t}_{k}.npy" for t in ("frame", "decoded") for k in ("bytes", "xxh32_16MiB", "head", "sample"))
    assert sum(os.path.getsize(tmp_path / "a" / nm) for nm in names) <= 64_000_000
    arrs = {}
    for nm in names:
        x, y = np.load(tmp_path / "a" / nm), np.load(tmp_path / "b" / nm)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and np.array_equal(x, y), nm
        arrs[nm[:-4]] = x
    # the arrays are the step's outputs: the decoded bytes are the input, the frame is the oracle's
    data = oracle.gen_synthetic(N, 42)
    want = oracle.compress_frame(data, oracle.params(7, False, True))

    def digests(b):
        return [xxhash.xxh32(b[i:i + (16 << 20)]).intdigest() for i in range(0, len(b), 16 << 20)]
    assert arrs["decoded_bytes"].tolist() == [N] and arrs["frame_bytes"].tolist() == [lines[0]["frame_bytes"]]
    assert arrs["decoded_xxh32_16MiB"].tolist() == digests(data)
    assert arrs["frame_xxh32_16MiB"].tolist() == digests(want)
    assert arrs["decoded_head"].astype(np.uint8).tobytes() == data[:1 << 20]
    assert arrs["frame_head"].astype(np.uint8).tobytes() == want[:1 << 20]
    assert arrs["decoded_sample"].shape == arrs["frame_sample"].shape == (1 << 21,)


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline():
    line = _bench("--steps", "1", "--warmup", "1", "--full", "--cpu-mib", "64")
    assert line["roundtrip_ok"] is True and line["ms_per_step"] > 0
    cpu = line["cpu_baseline"]
    assert cpu["unit"] == "GiB/s" and cpu["value"] > 0 and cpu["cores"] >= 1
    assert cpu["compress_GiBps"] > 0 and cpu["decompress_GiBps"] > 0
