"""The AES-GCM kernels that only an environment switch reaches.

NOISE_AEAD_GCM_SHAPE = w1024r1 | w1024r2 | w1024r2k8 forces the launch shape
of gcm_ragged_staged (the paired shapes are otherwise reached only from
65536 records on) and NOISE_AEAD_GCM_DUPLEX=staged selects gcm_duplex_staged
instead of gcm_duplex_fused.  Both are read once per process, so each value
runs in a fresh child (tests/aes_shapes_check.py); the duplex switch rides
with the last shape.

Each child, bit-exact against the oracle, FAST and +5-byte misaligned
layouts, table and constant-time GHASH: 1100 ragged records of mixed states,
lengths (0..600 and 0, 15, 16, 17, 1400, 4096) and AD, every sealed record;
an in-place open with every 37th record tampered (status, plaintext, the
rejected records' bytes exactly as given); an out-of-place open into 0x5A
(a rejected record's output is never written).  The duplex child adds
test_duplex_vs_oracle's check on ((1400, 300, 256), (1401, 513, 256)) and
((1, 256, 256), (4096, 256, 256)).
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "aes_shapes_check.py")


@pytest.mark.parametrize("shape,mode", [("w1024r1", "ragged"), ("w1024r2", "ragged"),
                                        ("w1024r2k8", "duplex")])
def test_forced_shape(gpu, shape, mode):
    env = dict(os.environ, NOISE_AEAD_GCM_SHAPE=shape)
    env.pop("NOISE_AEAD_GCM_DUPLEX", None)
    if mode == "duplex":
        env["NOISE_AEAD_GCM_DUPLEX"] = "staged"
    r = subprocess.run([sys.executable, HELPER, mode], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    words = r.stdout.split()
    # 4 ragged runs x 3 passes x 1100 records; the duplex cases add 2 x 1325
    assert words[:1] == ["ok"] and int(words[1]) == 13200 + (2650 if mode == "duplex" else 0)
