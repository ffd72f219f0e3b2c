"""Single-record CipherState calls through the resident worker (worker.hip).

`noise_cipherstate_encrypt_with_ad` / `_decrypt_with_ad` on one record take
the resident worker, not a kernel launch.  ChaChaPoly records of up to 63
units whose Poly1305 input is at most 256 blocks run the latency-first path
(four lanes per ChaCha block, a Poly1305 tree over one block per lane);
longer ones the multi-pass path (P ChaCha passes, G Poly1305 blocks per lane);
AES-GCM gcm_wide_record in place in LDS.  The record lengths come from two
sources: the hand-picked sample of tests/aead_gpu.py (worker_cases), and the cases that
tests/length_classes.py derives from the worker's own arithmetic (tree width,
Horner depth G, ChaCha passes P, the worker_fast_fits border, the transport's
chunks and raw tail), run by the test_worker_length_classes_* tests.  Every case is checked
byte for byte against the oracle (the restatement of
src/backend/ref/cipher-chachapoly.c:107-143 and cipher-aesgcm.c:156-188),
then opened back, then opened tampered: MAC failure, buffer and nonce left
as given (cipherstate.c:373-410).
"""
import os
import random
import subprocess
import sys

import pytest

from aead_gpu import worker_cases as _cases
from gpu_support import AES, CHACHA

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cipher", [CHACHA, AES])
def test_worker_single_records_vs_oracle(aead, gpu, oracle, cipher):
    rnd = random.Random(cipher)
    key = bytes(rnd.randrange(256) for _ in range(32))
    _, tx = aead.CipherState.new_by_id(cipher)
    _, rx = aead.CipherState.new_by_id(cipher)
    assert tx.init_key(key) == 0 and rx.init_key(key) == 0
    n0 = (1 << 32) - 3  # the counter crosses 2^32 inside the run
    assert tx.set_nonce(n0) == 0 and rx.set_nonce(n0) == 0
    n = n0
    for L, A in _cases():
        pt = bytes(rnd.randrange(256) for _ in range(L))
        ad = bytes(rnd.randrange(256) for _ in range(A))
        ct = tx.seal(pt, ad)
        assert ct == oracle.encrypt(cipher, key, n, pt, ad), (L, A)
        # tampered: MAC failure, buffer and nonce untouched
        bad = bytearray(ct)
        bad[rnd.randrange(len(bad))] ^= 1 << rnd.randrange(8)
        rc, back = rx.open(bytes(bad), ad)
        assert rc == aead.ERROR_MAC_FAILURE and back == bytes(bad), (L, A)
        assert rx.nonce == n
        rc, back = rx.open(ct, ad)
        assert rc == 0 and back == pt, (L, A)
        n += 1
        assert tx.nonce == n and rx.nonce == n
    # requests go to device memory on a large-BAR device, else host memory
    assert aead.lib().noise_aead_debug_worker_placement() in (1, 2)
    tx.free()
    rx.free()


@pytest.mark.parametrize("vram", ["0", "1"])
def test_worker_request_placement(aead, gpu, vram):
    """Both request placements: pinned host memory with
    12-byte chunks, and device memory written through the BAR with 8-byte
    stamped halves.  The placement is chosen once per process, so each runs
    in one child process (worker_mode_check.py) against the oracle."""
    env = dict(os.environ, NOISE_AEAD_WORKER_VRAM=vram)
    r = subprocess.run([sys.executable, "-u", os.path.join(os.path.dirname(__file__), "worker_mode_check.py")],
                       env=env, timeout=110, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    placement = int(r.stdout.split("placement")[-1].split()[0])
    assert placement == 1 if vram == "0" else placement in (1, 2)


@pytest.mark.parametrize("vram", ["0", "1"])
def test_worker_stream_head_edges(aead, gpu, vram):
    """The stream's head/tail boundary (worker_proto.h: the first 3072 stream
    bytes in host memory, 2048 in device memory, travel as stamped chunks,
    the rest raw): records whose stream total sits at head - 1 .. head + 17
    for both heads, both ciphers, AD 0 and 17, seal and open, in either
    placement (tests/worker_mode_check.py --head-edges)."""
    env = dict(os.environ, NOISE_AEAD_WORKER_VRAM=vram)
    r = subprocess.run([sys.executable, "-u", os.path.join(os.path.dirname(__file__), "worker_mode_check.py"),
                        "--head-edges"], env=env, timeout=110, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split("head_edges")[-1].split()[0]) == 72
    placement = int(r.stdout.split("placement")[-1].split()[0])
    assert placement == 1 if vram == "0" else placement in (1, 2)


def test_worker_in_place_buffer_semantics(aead, gpu, oracle):
    """encrypt_with_ad on a NoiseBuffer: size grows by 16, max_size checked
    first (cipherstate.c:299-333); the worker's fast path leaves bytes past
    the record's end alone."""
    import ctypes as C
    key = bytes(range(32))
    _, st = aead.CipherState.new_by_id(CHACHA)
    assert st.init_key(key) == 0
    L = 1000
    pt = bytes((7 * i) & 255 for i in range(L))
    mem = (C.c_uint8 * (L + 64)).from_buffer_copy(pt + bytes([0xAB]) * 64)
    nb = aead.NoiseBuffer.inout(mem, L, L + 16)
    assert st.encrypt_with_ad(b"", nb) == 0 and nb.size == L + 16
    assert bytes(mem)[:L + 16] == oracle.encrypt(CHACHA, key, 0, pt)
    assert bytes(mem)[L + 16:] == bytes([0xAB]) * 48
    st.free()


def _mode(args, env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-u", os.path.join(os.path.dirname(__file__), "worker_mode_check.py")] + args,
                       env=env, timeout=110, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _after(out, word):
    return int(out.split(word)[-1].split()[0])


@pytest.mark.parametrize("vram", ["0", "1"])
def test_worker_length_classes_chacha(gpu, vram):
    """Every case of the worker's own geometry (tests/length_classes.py):
    the 312 cases of worker_chacha_fast's tree and tail, both sides of
    worker_fast_fits's border for every AD length, the 160 records that reach
    worker_chacha_multi's 165 marginals (every G and P in 1..17) and the
    transport's cases for the placement in use, each sealed against the
    oracle, opened tampered and opened back, in either placement
    (tests/worker_mode_check.py --classes chacha)."""
    import length_classes as LC
    out = _mode(["--classes", "chacha"], {"NOISE_AEAD_WORKER_VRAM": vram})
    placement = _after(out, "placement")
    assert placement == 1 if vram == "0" else placement in (1, 2)
    transport = len({x[1:] for x in LC.full("wtransport", placement - 1)})
    assert _after(out, "classes") == 312 + 19 + 160 + transport


@pytest.mark.parametrize("vram,ct", [("0", "0"), ("1", "0"), ("1", "1")])
def test_worker_length_classes_aes(gpu, vram, ct):
    """gcm_wide_record in place in the worker's LDS over full("gcm_wide",
    ct): every case of the 8-chain deal, the lengths around EARLY and the
    seal's second round (M = 255, 256, 257: records over 4096 bytes, which
    test_worker_single_records_vs_oracle leaves out), with the tables in both
    placements and with the constant-time GHASH (NOISE_AEAD_CT_GHASH=1) in
    device memory where the device has it (tests/worker_mode_check.py
    --classes aes)."""
    import length_classes as LC
    out = _mode(["--classes", "aes"], {"NOISE_AEAD_WORKER_VRAM": vram, "NOISE_AEAD_CT_GHASH": ct})
    placement = _after(out, "placement")
    assert placement == 1 if vram == "0" else placement in (1, 2)
    assert _after(out, "classes") == len(LC.full("gcm_wide", 0, ct == "1"))


def test_worker_slot_serves_states_in_turn(gpu):
    """One slot serving three AES-GCM and two ChaChaPoly states in turn
    (tests/worker_mode_check.py --sequence): the two-entry cache of AES-GCM
    contexts evicts, a state is keyed again and one freed and replaced, short
    records follow long ones and seals follow rejected opens; calls with more
    AD than the worker takes go to the launch path with the same result."""
    out = _mode(["--sequence"], {})
    assert _after(out, "sequence") == 200 and _after(out, "big_ad") == 4
    assert min(_after(out, w) for w in ("evictions", "long_short", "reject_seal")) >= 1, out


def test_worker_calls_from_four_threads(gpu):
    """Four threads, each on its own states, 150 seal-then-open calls each
    over both ChaChaPoly paths and AES-GCM, every record against the oracle
    (tests/worker_mode_check.py --threads)."""
    out = _mode(["--threads"], {})
    assert _after(out, "calls") == 600 and _after(out, "mismatches") == 0
    assert _after(out, "served") == 4 and _after(out, "resident") >= 1, out


def _child(script, env_extra, timeout=110):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-u", os.path.join(os.path.dirname(__file__), script)],
                       env=env, timeout=timeout, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_batch_beside_resident_worker(gpu):
    """A C2-sized batch launched right after a single call (the worker still
    resident on its CU) takes the time of the same batch on a device with no
    worker: batch launches that fill every CU ask the workers to leave first
    (worker_park_for_batch).  The unparked cost is measured beside it
    (NOISE_AEAD_WORKER_PARK=0) and reported, not asserted."""
    import json
    parked = json.loads(_child("worker_batch_check.py", {}).strip().splitlines()[-1])
    unparked = json.loads(_child("worker_batch_check.py", {"NOISE_AEAD_WORKER_PARK": "0"})
                          .strip().splitlines()[-1])
    print("parked", parked["ratio"], "unparked", unparked["ratio"])
    assert max(parked["resident_before_warm"]) >= 1  # the single call did leave a worker
    # cold batches of 0.11 ms vary by +-5 % between launches: 1.10 separates
    # parked (measured 1.04-1.05) from unparked (1.36-1.43)
    assert parked["ratio"] <= 1.10, parked


def _tool(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "tools", name)
    if not os.path.exists(path):
        pytest.skip(f"tools/{name} not built (tools/build_latency.sh)")
    return path


def test_single_calls_scale_over_threads(gpu):
    """T threads on T CipherStates make T single calls at once (each thread
    takes a request slot of its own, as T CPU threads would each run the
    reference's cipherstate.c:293-410 without a lock): under the box's
    default environment (4 high-priority hardware queues) 8 threads reach at
    least 6x the call rate of one (tools/mt_calls: 1400-B encrypt + decrypt
    per iteration, every record checked).  The worker groups take 3 of the
    4 queues with 3 slots each (one worker per queue capped the
    device at 4 threads)."""
    import json
    tool = _tool("mt_calls")
    rates = {}
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "NOISE_AEAD_WORKER_QUEUES",
                                                           "NOISE_AEAD_WORKER_SLOTS")}
    for t in (1, 8):
        r = subprocess.run([tool, "chachapoly", str(t), "1400", "1.0"], timeout=60,
                           capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["ok"]
        rates[t] = d["calls_per_s"]
    print("calls/s", rates)
    assert rates[8] >= 6 * rates[1], rates


def test_other_streams_beside_resident_workers(gpu):
    """Work the application queues on its own streams does not wait for the
    resident workers: with 1 and 4 threads making single calls back to back,
    a memset on each of 8 newly created streams completes in well under a
    millisecond (tools/queue_probe).  A worker on a normal-priority stream
    shares a hardware queue with such streams and held them for its whole
    5 s lifetime; the workers' high-priority streams keep them apart, and of
    the high-priority queues the workers leave one to the application."""
    import json
    tool = _tool("queue_probe")
    # normal-priority application streams (8 of them), and one high-priority
    # stream of the application's own: the worker groups leave it the last
    # high-priority queue
    for workers, streams, prio in ((1, 8, "normal"), (4, 8, "normal"), (8, 8, "normal"), (4, 1, "high"),
                                   (8, 1, "high")):
        r = subprocess.run([tool, str(streams), str(workers), prio], timeout=60, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        d = json.loads(r.stdout.strip().splitlines()[-1])
        print(d)
        assert d["calls"] > 0
        assert max(d["memset_us"]) < 20000, d


def test_worker_launch_failure_falls_back(gpu):
    """A worker that cannot be launched (NOISE_AEAD_DEBUG_WORKER_FAIL=1) costs
    no call: every record takes the launch path with the same nonce and
    result (vs the oracle), nonces advance once per call, and the failed
    workers are retired."""
    out = _child("worker_mode_check.py", {"NOISE_AEAD_DEBUG_WORKER_FAIL": "1"})
    assert int(out.split("placement")[-1].split()[0]) == 0, out


def test_freed_aes_state_clears_worker_cache(gpu):
    """An AES-GCM state's context is cached in a worker's LDS by its single
    calls; freeing the state makes every worker that may hold it leave, and
    a leaving worker zeroes its LDS cache (worker.hip, after its loop).  The
    child runs with a 10 s idle timeout, so only the free can end it."""
    env = {"NOISE_AEAD_DEBUG_WORKER_IDLE_MS": "10000"}
    r = subprocess.run([sys.executable, "-u", os.path.join(os.path.dirname(__file__), "worker_mode_check.py"),
                        "--free-check"], env=dict(os.environ, **env), timeout=110, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("left_ms")[-1].split()[0]) >= 0


def test_free_beside_concurrent_caller_parks_only_that_worker(gpu):
    """freeing an AES-GCM state parks the worker that was sent its
    context even while another thread keeps writing request headers (the
    stop word has a chunk of its own), and only that worker — the other
    thread's worker, which never saw the context, is not relaunched (two
    groups of one slot: the two threads' slots are in different groups)."""
    env = {"NOISE_AEAD_DEBUG_WORKER_IDLE_MS": "10000", "NOISE_AEAD_WORKER_QUEUES": "2",
           "NOISE_AEAD_WORKER_SLOTS": "1"}
    r = subprocess.run([sys.executable, "-u", os.path.join(os.path.dirname(__file__), "worker_mode_check.py"),
                        "--free-concurrent"], env=dict(os.environ, **env), timeout=110, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "parked_ok 1" in r.stdout


def test_group_stays_while_one_slot_is_busy(gpu):
    """Worker groups (round 5): a group's workgroup leaves for idleness only
    when every slot of the group has been idle, so one thread's idle slot
    does not relaunch the group another thread keeps busy; with both quiet
    the group leaves by itself (tests/worker_mode_check.py --group-idle)."""
    env = {"NOISE_AEAD_WORKER_QUEUES": "1", "NOISE_AEAD_WORKER_SLOTS": "2", "NOISE_AEAD_DEBUG_WORKER_IDLE_MS": "20"}
    r = subprocess.run([sys.executable, "-u", os.path.join(os.path.dirname(__file__), "worker_mode_check.py"),
                        "--group-idle"], env=dict(os.environ, **env), timeout=110, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "group_idle_ok 1" in r.stdout


def test_relaunch_mid_wait_keeps_context_history(gpu):
    """a call whose group leaves after the call found it up and
    before its request was served relaunches the group from its wait loop;
    the relaunch starts the slot's context history afresh, so the call notes
    its AES-GCM context again.  Freeing the state then parks the relaunched
    group (NOISE_AEAD_DEBUG_WORKER_LEAVE=1 forces the race on every call;
    tests/worker_mode_check.py --relaunch-free)."""
    env = {"NOISE_AEAD_DEBUG_WORKER_IDLE_MS": "10000", "NOISE_AEAD_DEBUG_WORKER_LEAVE": "1"}
    r = subprocess.run([sys.executable, "-u", os.path.join(os.path.dirname(__file__), "worker_mode_check.py"),
                        "--relaunch-free"], env=dict(os.environ, **env), timeout=110, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "relaunch_free_ok 1" in r.stdout
