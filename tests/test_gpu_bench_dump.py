"""A plain bench.py run on the GPU and its --dump-outputs files.

A plain run (`--gpus 1 --steps N --warmup W`) prints the headline line
without the fields that take work of their own (roofline, per-direction
rates, checks, CPU baseline: `--full`), and `--dump-outputs DIR` writes what
the last timed step computed.  The dump is checked against the oracle: the
sampled sealed records are the oracle's ciphertext and tag of the step's
plaintext, the opened records are the plaintext of the set that step opened,
and the checksums of those records are the sums of the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "seal_gibs", "open_gibs", "verified", "verify", "cpu_baseline", "scatter_gather")


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(oracle, tmp_path):
    import bench

    steps, sets, lag = 3, 4, 2
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--settle-ms", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=150, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert "encrypt+decrypt, 64Ki x 1400B records per GPU" in d["metric"]
    # value and ms_per_step say the same thing: payload of one step / its time
    assert d["value"] == pytest.approx(d["config"]["payload_bytes_per_step"] / (d["ms_per_step"] * 1e-3) / 2**30,
                                       rel=1e-3)
    assert not [k for k in FULL_ONLY if k in d]

    files = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(files) == ["open_status", "opened_checksums", "opened_sample", "sample_records",
                             "sealed_checksums", "sealed_sample"]
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64_000_000

    c = bench.CONFIGS["c2"]
    N, L = c["records"], c["len"]
    in_stride = bench.stride(L, bench.SLOT_ALIGN)
    idx = files["sample_records"].astype(np.int64)
    assert np.array_equal(idx, bench.dump_sample(N, 1024))
    assert files["sealed_sample"].shape == (len(idx), L + 16)
    assert files["opened_sample"].shape == (len(idx), L)
    assert files["sealed_checksums"].shape == (N, 2) and files["opened_checksums"].shape == (N, 2)
    assert files["open_status"].shape == (N,) and not files["open_status"].any()

    key = oracle.fill(bench.SEED_KEY, 32, 0)
    b_seal, b_open = (steps - 1) % sets, (steps - 1 - lag) % sets

    def plaintext(b, i):  # record i of set b (bench.UniformWork: word0 of the set + the slot's words)
        return oracle.fill(bench.SEED_PT, L + 8, (b << 40) // 8 + i * in_stride // 8)[:L]

    weights = np.arange(1, L + 17, dtype=np.int64)
    for row in (0, 1, len(idx) // 2, len(idx) - 1):  # both ends of the batch and two drawn records
        i = int(idx[row])
        sealed = np.frombuffer(oracle.encrypt(bench.CHACHA, key, i, plaintext(b_seal, i)), dtype=np.uint8)
        assert np.array_equal(files["sealed_sample"][row], sealed.astype(np.float32)), i
        assert files["sealed_checksums"][i].tolist() == [int(sealed.sum()), int((sealed * weights).sum())]
        opened = np.frombuffer(plaintext(b_open, i), dtype=np.uint8)
        assert np.array_equal(files["opened_sample"][row], opened.astype(np.float32)), i
        assert files["opened_checksums"][i].tolist() == [int(opened.sum()), int((opened * weights[:L]).sum())]
