#!/usr/bin/env python3
"""bench.py — device-resident Noise transport AEAD throughput on MI355X.

Metric (BASELINE.json): GiB/s device-resident AEAD encrypt+decrypt of
64 Ki x 1400 B records per GPU.  One "step" = one seal pass (encrypt +
Poly1305/GHASH tag) over the batch followed by one open pass (verify + decrypt)
of the sealed batch, both through the C ABI of noise-c_amd
(noise_aead_dev_{seal,open}_uniform).  Payload processed per step per GPU =
2 x records x len (every byte goes through one AEAD op in each direction).
Inputs are resident in HBM before timing; the batch sets rotate so that the
working set (> 1 GiB) cannot be served from the 256 MiB Infinity Cache.

Multi-GPU: one process per GPU, records sharded by range with no data-path
collective — each rank seals/opens its own 64 Ki records of the global stream
(nonce base = rank x records): weak scaling.  Only the timing barrier and a
max-over-ranks all_reduce use the process group.  `--gpus N` without a
launcher starts the N ranks itself (a child torch.distributed.run over
127.0.0.1, before anything touches the GPU) and relays rank 0's line; under a
launcher WORLD_SIZE must equal --gpus.

A plain run sets up, settles and warms up, times the --steps steps, writes
the last step's outputs if --dump-outputs DIR is given, and prints the line
with the headline figure (metric, value, ms_per_step, the workload's config).
Everything else runs only with --full:

With --full, after the N-rank region rank 0 runs the same per-rank work alone
(the others wait at a barrier): that in-run N = 1 value gives
per_gpu_efficiency.

With --full every run verifies after its timed region: every open status 0,
every opened record equal to its plaintext, and the records the timed kernels
sealed (set 0 of this rank's shard) hashing to the golden digest of
tests/golden/shard_digests.json ("verified" in the line).  It also times each
direction's (C5: each kernel's) launches in a pass of their own for the
roofline fields and, with a process group, the scatter/seal/gather leg.

The CPU baseline (--full) is the reference noise-c itself (oracle/_ref/ref_bench:
the reference's CipherState API compiled from its own sources), timed on this
host's cores on a bounded sample of the same workload.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "noise-c_amd"))

CHACHA, AES = 0x4301, 0x4302
GIB = float(1 << 30)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec, MI355X_MICROARCH.md chip table

CONFIGS = {
    # name: cipher, records per GPU, record length, key states per GPU
    "c2": dict(cipher=CHACHA, records=65536, len=1400, states=1,
               workload="ChaCha20-Poly1305 64Ki x 1400B records, one CipherState key"),
    "c3": dict(cipher=AES, records=65536, len=1400, states=1,
               workload="AES-256-GCM 64Ki x 1400B records, one CipherState key"),
    # C4: 1 Mi records / 4096 states IN TOTAL, sharded by state
    # block over the ranks (strong scaling)
    "c4": dict(cipher=CHACHA, records=1048576, len=1400, states=4096, strong=True,
               workload="ChaCha20-Poly1305 1Mi x 1400B records, 4096 CipherStates x 256"),
    # noise-c's own tests/performance perf_cipher shape (test-performance.c
    # :140-179): 1024-B records with 32 B of associated data each
    "perf": dict(cipher=CHACHA, records=65536, len=1024, states=1, ad=32,
                 workload="ChaCha20-Poly1305 64Ki x 1024B records + 32B AD (tests/performance shape)"),
    # C5 per GPU = 1/8 of the 8-GPU job (1 Mi records, 4096 states in total):
    # lengths 64 + splitmix64(seed_len + i) mod 16321, cipher by state parity.
    "c5": dict(cipher=None, records=131072, len=None, states=512, mixed=True,
               workload="Mixed ChaChaPoly (even states) + AESGCM (odd states), 64 B-16 KiB "
                        "records (SURVEY.md 8d C5), 128 Ki records / 512 CipherStates per GPU, "
                        "ragged descriptors"),
    # C5's layout rule at 1/8 of its records per GPU (256 records per state as
    # in C5): the multi-rank rehearsal of the ragged path in the GPU tests
    # (tests/test_gpu_rccl.py), with its own golden shard digests.  Not a
    # bench line.
    "c5s": dict(cipher=None, records=16384, len=None, states=64, mixed=True,
                workload="C5's mixed ChaChaPoly + AESGCM 64 B-16 KiB layout, reduced to 16 Ki records / "
                         "64 CipherStates per GPU (multi-rank rehearsal)"),
}
SEED_LEN, SEED_PT, SEED_KEY = 0x6C656E, 0x7074, 0x6B6579
# NOISE_BENCH_REHEARSE=1: rehearse the N>1 code path on a one-GPU box — every
# rank on cuda:0, gloo process group, collectives on CPU copies.  Only the
# transport differs from the real run (RCCL refuses two ranks on one GPU).
REHEARSE = os.environ.get("NOISE_BENCH_REHEARSE") == "1"


def cpu_if_rehearsal(t):
    return t.cpu() if REHEARSE else t
# Device record slots: strides roundup(len, SLOT_ALIGN) / roundup(len + 16,
# SLOT_ALIGN).  Whole 128-B lines per slot keep a record's first and last
# lines its own: with 16-B slots (1408 / 1424 B at 1400 B) the open re-read
# the line shared with the neighbouring record and the tag's line (duplex HBM
# bytes 1.13x vs 1.10x algorithmic); +0.6-0.8 % at C2/C3/C4 in three
# interleaved rounds (profiles/r02/align_all_ab.jsonl).  DESIGN.md §3.
IN_ALIGN = 16
SLOT_ALIGN = 128


def shard(records_per_gpu: int, states: int, rank: int, world: int):
    """Records of rank `rank` in the global stream (weak scaling): the rank's
    records are [rank*R, (rank+1)*R); with S states per GPU, global state
    rank*S + s owns records rank*R + s*(R/S) ... and its nonces start at 0.
    With a single state per GPU the ranks share one logical CipherState whose
    nonce runs across the ranks' ranges (nonce base = rank*R)."""
    first = rank * records_per_gpu
    rps = records_per_gpu // states
    if states == 1:
        nonce_base = [first]
    else:
        nonce_base = [0] * states
    key_ids = [rank * states + s for s in range(states)] if states > 1 else [0]
    return dict(first=first, count=records_per_gpu, rps=rps, nonce_base=nonce_base,
                key_ids=key_ids)


def splitmix64_np(x):
    """SplitMix64 of uint64 array x (oracle_splitmix64)."""
    import numpy as np
    with np.errstate(over="ignore"):
        z = x.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def mixed_layout(records_per_gpu: int, states: int, rank: int):
    """C5 shard of rank: global record i = rank*R + j, length
    64 + splitmix64(SEED_LEN + i) % 16321, state rank*S + j // (R/S),
    ChaChaPoly for even global states, AESGCM for odd; record slots are
    roundup64(len + 16) bytes (FAST: 16-B aligned, readable past the tag)."""
    import numpy as np
    R, S = records_per_gpu, states
    gi = np.arange(rank * R, (rank + 1) * R, dtype=np.uint64)
    lens = (np.uint64(64) + splitmix64_np(np.uint64(SEED_LEN) + gi) % np.uint64(16321)).astype(np.int64)
    slot = (lens + 16 + 63) // 64 * 64
    off = np.zeros(R, dtype=np.int64)
    off[1:] = np.cumsum(slot)[:-1]
    rps = R // S
    st_local = np.arange(R) // rps
    st_global = rank * S + st_local
    nonce = (np.arange(R) % rps).astype(np.uint64)
    return dict(lens=lens, off=off, total=int(off[-1] + slot[-1]), st_local=st_local,
                st_global=st_global, nonce=nonce, rps=rps)


def stride(n: int, align: int = IN_ALIGN) -> int:
    return (n + align - 1) // align * align


def physical_cores(cpus):
    """Distinct physical cores (package, core id) among the logical CPUs."""
    seen = set()
    for c in cpus:
        base = f"/sys/devices/system/cpu/cpu{c}/topology/"
        try:
            with open(base + "physical_package_id") as f:
                pkg = f.read().strip()
            with open(base + "core_id") as f:
                core = f.read().strip()
        except OSError:
            return None
        seen.add((pkg, core))
    return len(seen) or None


def host_cpu():
    """CPU model, logical CPUs, the affinity set, its physical cores and the
    CPU share this job is given (SURVEY.md 8d asks for the core count)."""
    model = None
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        aff = sorted(os.sched_getaffinity(0))
    except AttributeError:
        aff = list(range(os.cpu_count() or 1))
    share = os.environ.get("OMP_NUM_THREADS")
    return {"cpu_model": model, "nproc": os.cpu_count(), "usable_cpus": len(aff),
            "physical_cores": physical_cores(aff),
            "cpu_share": int(share) if share and share.isdigit() else None}


def cpu_baseline(cfg, budget_cpu_s: float = 12.0):
    """Reference noise-c on this host's cores, bounded sample."""
    r = _cpu_baseline(cfg, budget_cpu_s)
    return None if r is None else {**r, **host_cpu()}


def ref_perf_cipher(path, timeout_s=120.0):
    """Run the reference's tests/performance program (oracle/_ref/
    test-performance, built from its own sources) and read its ChaChaPoly and
    AESGCM perf_cipher lines (MiB/s; test-performance.c:140-179, 420-422).
    It goes on to time DH and signatures, which this baseline does not need:
    once both cipher lines are out the child is stopped (by its own PID)."""
    p = subprocess.Popen([path], stdout=subprocess.PIPE, text=True)
    out, t0 = {}, time.time()
    try:
        for line in p.stdout:
            f = line.split()
            if len(f) >= 3 and f[0] in ("ChaChaPoly", "AESGCM"):
                out[f[0]] = float(f[1])
            if len(out) == 2 or time.time() - t0 > timeout_s:
                break
    finally:
        p.kill()
        p.wait()
    return out


def _cpu_baseline(cfg, budget_cpu_s):
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_bench")
    kind = "reference"
    if not os.path.exists(ref):
        ref = os.path.join(ROOT, "oracle", "_build", "port_bench")
        kind = "port"
    if not os.path.exists(ref):
        return None
    cname = "aesgcm" if cfg["cipher"] == AES else "chachapoly"
    if cfg.get("ad"):
        # the reference's own tests/performance program, unchanged: 1 thread,
        # 200 MiB of 1024-B records with 32 B AD, encrypt only, CPU-time clock
        tp = os.path.join(ROOT, "oracle", "_ref", "test-performance")
        if os.path.exists(tp):
            r = ref_perf_cipher(tp)
            name = "AESGCM" if cfg["cipher"] == AES else "ChaChaPoly"
            return {"value": round(r[name] / 1024.0, 4), "unit": "GiB/s", "cores": 1,
                    "kind": "reference",
                    "sample": f"noise-c tests/performance/test-performance (built from the reference's "
                              f"sources, run unchanged): perf_cipher {name}, 200 MiB of 1024 B + 32 B AD "
                              f"encrypts, one thread, CPU-time clock (encrypt only); its AESGCM/ChaChaPoly "
                              f"lines: {r}"}
        out = subprocess.run([ref, "perf", cname, str(cfg["len"]), "200000", "1"],
                             capture_output=True, text=True, timeout=300, check=True)
        r = json.loads(out.stdout)
        return {"value": round(r["mib_per_s"] / 1024.0, 4), "unit": "GiB/s", "cores": 1,
                "kind": kind, "sample": f"{'reference library' if kind == 'reference' else 'oracle port'} "
                f"in a restatement of perf_cipher's loop (oracle/ref_bench.c perf; the reference's "
                f"test-performance binary was not built): 200000 x 1024 B + 32 B AD encrypts, one "
                f"thread, CPU-time clock (encrypt only)"}
    hc = host_cpu()
    usable, phys = hc["usable_cpus"], hc["physical_cores"] or hc["usable_cpus"]
    # one thread per physical core of the affinity set, within the CPU share
    # this job is given on the box (OMP_NUM_THREADS: 16 of the host's cores
    # per GPU on the pool; other jobs share the host)
    threads = max(1, min(phys, usable, hc["cpu_share"] or phys))
    # calibrate on one thread (~0.3 s), then size the sample to the budget
    probe_n = 200 if cfg["cipher"] == AES else 2000
    out = subprocess.run([ref, "roundtrip", cname, str(cfg["len"]), str(probe_n), "1"],
                         capture_output=True, text=True, timeout=120, check=True)
    p = json.loads(out.stdout)
    rec_per_s = probe_n / max(p["seconds"], 1e-6)
    per_thread = max(probe_n, int(rec_per_s * budget_cpu_s / threads))
    out = subprocess.run([ref, "roundtrip", cname, str(cfg["len"]), str(per_thread),
                          str(threads)], capture_output=True, text=True, timeout=600, check=True)
    r = json.loads(out.stdout)
    one = subprocess.run([ref, "roundtrip", cname, str(cfg["len"]), str(max(probe_n, int(rec_per_s * 2))), "1"],
                         capture_output=True, text=True, timeout=120, check=True)
    r1 = json.loads(one.stdout)
    res = {"value": round(r["gib_per_s"], 4), "unit": "GiB/s", "cores": threads, "kind": kind,
           "single_thread": round(r1["gib_per_s"], 4),
           "sample": (f"{'noise-c ref backend CipherState API' if kind == 'reference' else 'oracle restatement'}"
                      f" {cname}: {threads} threads (one per physical core, within this job's CPU share) x "
                      f"{per_thread} records x {cfg['len']} B, each encrypted then decrypted+verified "
                      f"(send/recv CipherState pair per thread), wall clock; 1 thread: "
                      f"{r1['gib_per_s']:.3f} GiB/s"),
           "ok": r["ok"]}
    if phys > threads:
        # not run (the box gives this job `threads` cores): per-thread rate x
        # the affinity set's physical cores, an upper bound for linear scaling
        res["all_physical_cores_linear_estimate"] = round(r["gib_per_s"] / threads * phys, 3)
    return res


def kernel_name(cipher, n, rps, lanes, in_stride, out_stride, length, duplex=False, ct=False):
    """The kernel the library dispatches for this uniform job's seal
    (aead_api.hip run_uniform) or, duplex, for the whole step (run_duplex), as
    rocprofv3 names it."""
    fast = in_stride % 16 == 0 and out_stride % 16 == 0 and in_stride >= (max(length, 1) + 63) // 64 * 64
    if cipher == CHACHA and fast and lanes == 1:  # one lane per record (seal_solo_staged)
        return f"chachapoly_{'duplex' if duplex else 'seal'}_solo<{'true' if rps % 64 == 0 else 'false'}>"
    if duplex and cipher == CHACHA and fast and lanes in (4, 8):
        return f"chachapoly_duplex_staged<{lanes}, {'true' if rps % (64 // lanes) == 0 else 'false'}>"
    if cipher == AES:
        c = "true" if ct else "false"
        if fast and rps % 256 == 0:
            if duplex:  # launch_aes.hip aes_duplex: the fused kernel unless told otherwise
                staged = os.environ.get("NOISE_AEAD_GCM_DUPLEX") == "staged"
                return f"gcm_duplex_{'staged' if staged else 'fused'}<{c}>"
            return f"gcm_staged<false, {c}>"
        return f"gcm_uniform<false, {c}>"
    if fast and lanes >= 4:
        return f"chachapoly_seal_staged<{lanes}, {'true' if rps % (64 // lanes) == 0 else 'false'}>"
    return f"chachapoly_seal_uniform<{lanes}, {'true' if fast else 'false'}>"


def load_pmc(config_name: str, kernel: str, scale: float = 1.0):
    """Per-launch PMC counters of `kernel` from profiles/traffic_<cfg>.json
    (tools/gpu/pmc.sh + tools/pmc_report.py, collected at N = 1), or {}.
    `scale`: this launch's share of the profiled one (1/N for a strong-scaling
    shard; the counters are per-launch totals proportional to the records)."""
    path = os.path.join(ROOT, "profiles", f"traffic_{config_name}.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        t = json.load(f)
    k = t.get("kernels", {}).get(kernel) or {}
    return {n: v * scale for n, v in k.items()} if scale != 1.0 else k


# VALU issue ceiling.  MI355X_MICROARCH.md: a SIMD-32 issues a
# wave64 VALU instruction over 2 cycles, so the chip-wide ceiling is 1024
# SIMDs x 2.4 GHz / 2 wave-instructions per second — reached only by the
# fast integer class (v_add/v_xor/v_bitop3).  Shifts, rotates and multiplies
# take ~4 cycles (profiles/r01_rates*.log), and a stream mixing the classes
# in one wave ran at ~4 (r01_runs_mix.log) until round 6 issued ChaCha in
# runs with priority toggles (aead_device.h chacha20_2block_runs); the line
# reports both the 2-cycle ceiling and round 1-5's 4-cycle one.
VALU_ISSUE_PEAK = 1024 * 2.4e9 / 2
VALU_ISSUE_PEAK_SLOW = 1024 * 2.4e9 / 4


def issue_bound(pmc, avg_launch_ms):
    n = pmc.get("SQ_INSTS_VALU")
    if not n or not avg_launch_ms:
        return None
    rate = n / (avg_launch_ms * 1e-3)
    return {"resource": "VALU issue (wave-instructions/s)", "valu_insts_per_launch": int(n),
            "achieved": round(rate / 1e9, 1), "peak": round(VALU_ISSUE_PEAK / 1e9, 1),
            "unit": "G wave-instr/s", "frac": round(rate / VALU_ISSUE_PEAK, 4),
            "frac_of_4cycle_issue": round(rate / VALU_ISSUE_PEAK_SLOW, 4),
            "source": "SQ_INSTS_VALU from the committed PMC profile / live launch time; peak = 2 cycles "
                      "per wave64 instruction on a SIMD-32 (MI355X_MICROARCH.md)"}


# The stream rank 0's one JSON line goes to.  A run with a process group
# points file descriptor 1 at stderr (keep_stdout_for_line): RCCL prints its
# version banner on stdout when a communicator is made, and the line must be
# the only thing there.
LINE_OUT = None  # None: sys.stdout as it is at the time of the line


def keep_stdout_for_line():
    global LINE_OUT
    sys.stdout.flush()
    LINE_OUT = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)


def emit_line(result):
    print(json.dumps(result), file=LINE_OUT or sys.stdout, flush=True)


def launch_ranks(n: int) -> int:
    """`--gpus N` (N > 1) without a launcher: run this script as N ranks of a
    child torch.distributed.run on 127.0.0.1 and return its exit status.  The
    child is started before this process touches the GPU, and this process
    never execs (MI355X pool rule)."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)]
    # stdout carries exactly rank 0's JSON line; whatever else the ranks or
    # their libraries print there (gloo's connection banner, ...) goes to stderr
    proc = subprocess.Popen(cmd + sys.argv[1:], stdout=subprocess.PIPE, text=True)
    for line in proc.stdout:
        if line.lstrip().startswith('{"metric"'):
            sys.stdout.write(line)
            sys.stdout.flush()
        else:
            sys.stderr.write(line)
    return proc.wait()


# C5's two streams when made before the process group (main)
C5_STREAMS = []


def init_dist(world, local, dry_run):
    import torch.distributed as dist
    if REHEARSE or dry_run:
        dist.init_process_group("gloo")
    else:
        import torch
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    return dist


def max_over_ranks(dist, torch, dev, x: float) -> float:
    if dist is None:
        return x
    t = torch.tensor([x], dtype=torch.float64, device=dev)
    t = cpu_if_rehearsal(t)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def dry_run(args, rank, world):
    """--dry-run: the N-rank plumbing with no GPU work — self-launch, the
    process group (gloo), the barrier / max-over-ranks timing and the rank-0
    line.  For CPU tests of the launcher; it reports no throughput."""
    import torch
    dist = init_dist(world, 0, True) if world > 1 else None
    if dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    elapsed = max_over_ranks(dist, torch, None, time.perf_counter() - t0)
    result = {"metric": "dry run (no GPU work)", "value": None, "unit": "GiB/s", "n_gpus": world,
              "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed * 1e3 / max(1, args.steps),
              "dry_run": True, "rank_env": {"WORLD_SIZE": os.environ.get("WORLD_SIZE"),
                                             "MASTER_ADDR": os.environ.get("MASTER_ADDR")}}
    if rank == 0:
        emit_line(result)
    if dist:
        dist.destroy_process_group()


def shard_golden(config: str, rank: int, world: int, strong: bool):
    """The golden sealed-record digest of this rank's set-0 shard
    (tests/golden/shard_digests.json), or None."""
    path = os.path.join(ROOT, "tests", "golden", "shard_digests.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        c = json.load(f)["configs"].get(config, {})
    if strong:
        return (c.get("world_rank_sealed_sha256", {}).get(str(world)) or [None] * (rank + 1))[rank]
    d = c.get("rank_sealed_sha256") or []
    return d[rank] if rank < len(d) else None


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None,
                    help="ranks (one per GPU); without a launcher bench.py starts them itself; "
                         "under one it must equal WORLD_SIZE (default: WORLD_SIZE, else 1)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--lanes", type=int, default=0, help="lanes per record (0 = library default)")
    ap.add_argument("--sets", type=int, default=4, help="rotating batch sets (> MALL)")
    ap.add_argument("--settle-ms", type=float, default=500.0,
                    help="untimed back-to-back steps before the warmup, in ms of wall clock "
                         "(the sustained-load clock, see settle()); 0 = off")
    ap.add_argument("--align", type=int, default=SLOT_ALIGN, choices=(16, 64, 128, 256),
                    help="record slot alignment of the device batch (strides roundup(len, align), "
                         "roundup(len + 16, align))")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run everything beside the headline figure: the "
                         "after-timing checks (statuses, round trip, golden digest), the per-direction "
                         "and per-kernel passes behind the roofline, the CPU baseline and, with a process "
                         "group, the scatter/seal/gather leg and the in-run N = 1 reference")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step computed (sealed records, "
                         "opened records, open statuses) as DIR/<name>.npy (UniformWork.dump, dump_mixed)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-verify", action="store_true",
                    help="--full: skip the after-timing checks (statuses, round trip, golden digest)")
    ap.add_argument("--verify", action="store_true", help=argparse.SUPPRESS)  # on by default now
    ap.add_argument("--no-xfer", action="store_true",
                    help="--full: skip the N>1 scatter/seal/gather leg (RCCL, SURVEY.md 8e)")
    ap.add_argument("--xfer-reps", type=int, default=5)
    ap.add_argument("--no-n1", action="store_true",
                    help="--full, N > 1: skip the in-run N = 1 reference (rank 0 alone) behind "
                         "per_gpu_efficiency")
    ap.add_argument("--n1-value", type=float, default=None,
                    help="N = 1 value of the same config from another run (overrides the in-run one)")
    ap.add_argument("--mode", default="duplex", choices=("duplex", "separate", "seal"),
                    help="duplex: each step seals one set and opens another in ONE launch "
                         "(noise_aead_dev_duplex_uniform); separate: a seal launch then an open launch; "
                         "seal: encrypt only, one standalone seal launch per step (the north star's "
                         "literal metric: device-resident ChaCha20-Poly1305 encrypt, C2-C4/perf)")
    ap.add_argument("--events", default="ends", choices=("ends", "step"),
                    help="ends: HIP events only around the timed region (per-launch time = "
                         "its interval / launches); step: events at every launch boundary")
    ap.add_argument("--streams", type=int, default=1, choices=(1, 2),
                    help="C2-C4/perf: 2 = consecutive steps alternate between two streams")
    ap.add_argument("--ct-ghash", action="store_true",
                    help="AES-GCM: NOISE_AEAD_FLAG_CT_GHASH (table-free GHASH)")
    ap.add_argument("--verify-first", action="store_true",
                    help="opens with NOISE_AEAD_FLAG_VERIFY_FIRST (authenticate, then decrypt): the "
                         "default open order since round 6, kept as an explicit no-op")
    ap.add_argument("--one-pass", action="store_true",
                    help="ChaChaPoly opens with the opt-in NOISE_AEAD_FLAG_ONE_PASS (decrypt while "
                         "authenticating; a rejected record's plaintext is undone before the kernel ends)")
    ap.add_argument("--c5-streams", type=int, default=2, choices=(1, 2),
                    help="C5: 2 = the AES-GCM and ChaChaPoly halves on two streams, concurrently")
    ap.add_argument("--c5-prio", default="none", choices=("none", "aes", "chacha"),
                    help="C5 with two streams: the half whose stream is high-priority")
    ap.add_argument("--c5-sets", type=int, default=1, choices=(1, 2),
                    help="C5 with two streams and --c5-join step: 2 = each step seals one set and opens "
                         "the set sealed the step before (four independent launches, as C2-C4's duplex)")
    ap.add_argument("--c5-first", default="aes", choices=("aes", "chacha"),
                    help="C5 with two streams and --c5-join step: the half launched first")
    ap.add_argument("--c5-join", default="step", choices=("step", "phase"),
                    help="C5 with two streams: each cipher's open follows its own seal and the halves "
                         "join once per step (step), or both seals finish before either open (phase)")
    ap.add_argument("--rccl", action="store_true",
                    help="form the nccl (RCCL) process group and run the max-over-ranks timing and, with "
                         "--full, the scatter/seal/gather leg through it even at WORLD_SIZE=1 (a one-GPU "
                         "check of the N > 1 code path on RCCL; the value is the N = 1 value)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / process-group plumbing only, no GPU work (CPU tests)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def main():
    args = parse_args()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and (args.gpus or 1) > 1:
        sys.exit(launch_ranks(args.gpus))
    world = int(env_world or 1)
    if args.rccl and env_world is None:  # a one-rank group without a launcher
        import socket
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1",
                          MASTER_PORT=str(port))
    if args.gpus is not None and args.gpus != world:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 or args.rccl:
        keep_stdout_for_line()
    if args.dry_run:
        return dry_run(args, rank, world)

    import torch
    import noise_aead as A

    dist = None
    if REHEARSE:
        local = 0
    if world > 1 or args.rccl:
        torch.cuda.set_device(local)
        if CONFIGS[args.config].get("mixed") and args.c5_streams == 2:
            # HIP binds a stream to one of the process's GPU_MAX_HW_QUEUES (4)
            # hardware queues at the stream's first use.  First used after
            # RCCL's streams, C5's two streams shared one queue and the halves
            # ran one after the other (step 2.09 -> 2.43 ms; the kernel trace's
            # Queue_Id, profiles/r05/rccl_one_rank.txt); used once here, before
            # the process group, they own two queues
            C5_STREAMS[:] = [torch.cuda.Stream(torch.device("cuda", local)) for _ in range(2)]
            for st_ in C5_STREAMS:
                with torch.cuda.stream(st_):
                    torch.zeros(1, device=torch.device("cuda", local)).add_(1)
            torch.cuda.synchronize()
            torch.cuda.set_stream(C5_STREAMS[0])
        dist = init_dist(world, local, False)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    cfg = CONFIGS[args.config]
    if cfg.get("mixed"):
        return run_mixed(args, cfg, A, torch, dev, rank, world, dist)
    N, S = cfg["records"], cfg["states"]
    if cfg.get("strong"):
        if N % world or S % world:
            raise SystemExit(f"{args.config}: {N} records / {S} states do not split over {world} ranks")
        N, S = N // world, S // world
    wl = UniformWork(args, cfg, A, torch, dev, N, S, shard(N, S, rank, world))
    elapsed = wl.timed(args.steps, args.warmup, dist)
    # the per-direction pass right after the timed region, at the clock it
    # left (it used to follow verify()'s D2H and SHA-256,
    # an idle GPU); its outputs go to scratch buffers, so what verify()
    # checks is still only what the timed launches wrote
    seal_ms, open_ms = wl.per_direction_ms() if args.full else (None, None)
    elapsed = max_over_ranks(dist, torch, dev, elapsed)
    if dist:
        dist.barrier()
    if args.dump_outputs:
        wl.dump(dump_dir(args, rank, world))
    verify = verify_over_ranks(dist, torch, dev,
                               wl.verify(args.config, rank, world) if args.full and not args.no_verify else None)

    L, AD = wl.L, wl.AD
    payload_step = wl.dirs * N * L * world                     # both directions (seal mode: one), all ranks
    value = payload_step * args.steps / elapsed / GIB
    S_all = S * world
    op = "encrypt" if wl.seal_only else "encrypt+decrypt"
    result = {
        "metric": (f"GiB/s device-resident AEAD {op}, {N * world // 1024}Ki x {L}B "
                   f"records in total over {S_all} CipherStates, sharded by state"
                   if cfg.get("strong") else
                   f"GiB/s device-resident AEAD {op}, {N // 1024}Ki x {L}B records"
                   + (f" + {AD}B AD" if AD else "") + " per GPU"),
        "value": round(value, 2),
        "unit": "GiB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed * 1e3 / args.steps, 4),
        "higher_is_better": True,
        "scaling": "strong" if cfg.get("strong") else "weak",
        "vs_baseline": None,
        "dtype": "u32",
        "data": "synthetic (SplitMix64 plaintext and keys, SURVEY.md 8d), resident in HBM",
        "config": {"workload": cfg["workload"], "config": args.config, "records_per_gpu": N,
                   "record_len": L, "states_per_gpu": S, "lanes_per_record": wl.lanes,
                   "in_stride": wl.in_stride, "out_stride": wl.out_stride,
                   "payload_bytes_per_step": int(payload_step), "parallelism": f"records x{world}",
                   "streams": len(wl.streams), "mode": args.mode, "events": args.events,
                   "open_reads_set_sealed_steps_before": wl.lag,
                   "settle": {"ms": args.settle_ms, "steps": wl.settle_steps,
                              "s": round(wl.settle_s, 3)},
                   "open_order": ("verify-first (the default: authenticate, then decrypt verified "
                                  "records; cipher-chachapoly.c:135-141, cipher-aesgcm.c:172-188)"
                                  if wl.vf else
                                  "one pass (NOISE_AEAD_FLAG_ONE_PASS: decrypt while authenticating; "
                                  "a rejected record's plaintext is undone before the kernel ends)"),
                   **({"ct_ghash": True} if args.ct_ghash else {})},
    }
    if args.full:
        uniform_full(args, cfg, A, torch, dev, rank, world, dist, wl, N, S, seal_ms, open_ms, verify, result)
    finish(args, result, rank, world, dist)


def dump_dir(args, rank, world):
    """--dump-outputs DIR: one rank writes into DIR itself, rank r of several
    into DIR/rank<r>."""
    return args.dump_outputs if world == 1 else os.path.join(args.dump_outputs, f"rank{rank}")


def uniform_full(args, cfg, A, torch, dev, rank, world, dist, wl, N, S, seal_ms, open_ms, verify, result):
    """--full, uniform configs: adds to `result` the line's fields beside the
    headline figure (roofline, per-direction rates, checks, the
    scatter/seal/gather leg, the in-run N = 1 reference, the CPU baseline)."""
    L, AD = wl.L, wl.AD
    alg_seal = N * (2 * L + 16 + AD) + len(wl.sh["key_ids"]) * 40  # SURVEY §8d algorithmic bytes (+AD read)
    # a VERIFY_FIRST open shares the duplex launch only with the one-lane
    # ChaChaPoly and the staged AES-GCM kernels (aead_api.hip run_duplex);
    # otherwise a step is two launches
    vf_duplex = "_duplex_" in kernel_name(wl.cipher, N, wl.sh["rps"], wl.lanes, wl.in_stride,
                                          wl.out_stride, L, True, args.ct_ghash) and \
        (wl.cipher == AES or wl.lanes == 1)
    two_launch = wl.duplex and wl.vf and not vf_duplex
    kname = kernel_name(wl.cipher, N, wl.sh["rps"], wl.lanes, wl.in_stride, wl.out_stride, L,
                        wl.duplex and not two_launch, args.ct_ghash)
    if two_launch:
        alg_launch, launch_ms_ = alg_seal, wl.launch_ms / 2
    elif "_duplex_" in kname:
        # the one launch of a step: one seal + one open of N records each
        alg_launch, launch_ms_ = 2 * alg_seal, wl.launch_ms
    elif not wl.duplex and not wl.per_step:
        # seal and open alternate: the mean interval per launch, gaps included
        alg_launch, launch_ms_ = alg_seal, wl.launch_ms
    else:
        alg_launch, launch_ms_ = alg_seal, seal_ms
    achieved = alg_launch / (launch_ms_ * 1e-3) / 1e9
    # the committed PMC profiles are of the default open order (verify
    # first since round 6; profiles/traffic_<cfg>.json), of the standalone
    # seal for --mode seal (traffic_<cfg>_seal.json)
    pmc = {} if args.one_pass and wl.cipher != AES else \
        load_pmc(args.config + ("_seal" if wl.seal_only else ""), kname,
                 1.0 / world if cfg.get("strong") else 1.0)
    traffic = pmc.get("hbm_bytes_per_launch")
    result["config"]["per_direction"] = ("seal_gibs / open_gibs: 20 standalone launches each, right after "
                                         "the timed region (settled clock), outputs to scratch buffers")
    result.update({
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                     "traffic": traffic, "kernel": kname,
                     "algorithmic_bytes_per_launch": alg_launch,
                     "avg_launch_ms": round(launch_ms_, 5),
                     "issue_bound": issue_bound(pmc, launch_ms_)},
        "seal_gibs": round(N * L * world / (seal_ms * 1e-3) / GIB, 2),
        "open_gibs": round(N * L * world / (open_ms * 1e-3) / GIB, 2),
        "open_roofline_frac": round(alg_seal / (open_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
    })
    if verify is not None:
        result["verified"] = verify.pop("ok")
        result["verify"] = verify
    if dist is not None and not args.no_xfer:
        try:  # reported beside the value; a failure here never voids the bench line
            result["scatter_gather"] = xfer_leg(args, torch, dist, dev, A, rank, world, N, L,
                                                wl.in_stride, wl.out_stride, wl.sh, wl.sets, wl.seal)
        except Exception as e:
            result["scatter_gather"] = {"error": repr(e)}
        # a failed scatter/gather is stated at the top level of
        # the line (it still never voids the GPU number)
        sgr = result["scatter_gather"]
        result["scatter_gather_ok"] = "error" not in sgr and bool(sgr.get("verified", sgr.get("ok", False)))
    if world > 1 and not args.no_n1 and args.n1_value is None:
        result["n1_in_run"] = n1_reference(args, cfg, A, torch, dev, rank, dist, wl, N, S, world)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            result["cpu_baseline"] = cpu_baseline(cfg)
        except Exception as e:  # reported, never fatal to the GPU number
            result["cpu_baseline"] = {"error": str(e)}


def settle(torch, dev, stream, ms, step):
    """Run the workload's own step back to back for `ms` of wall clock before
    the warmup steps, keeping 8-32 steps queued (no idle GPU between chunks),
    so the timed steps see the clock the chip holds under sustained load.
    Under a VALU-dense load MI355X first boosts, drops to ~1.9 GHz after
    ~5 ms, then climbs back to ~2.4 GHz over ~0.1-0.3 s (C2-shaped duplex
    launch, tools/microbench/timeline3: 2.03 GHz after 10 launches, 1.90 after
    40, 2.33 after 200, 2.44 after 2000; profiles/r03/clock_vs_warmup.log).
    Returns (steps run, seconds)."""
    if ms <= 0:
        return 0, 0.0
    t0 = time.perf_counter()
    t_end = t0 + ms * 1e-3
    n, chunk, prev = 0, 16, None
    while True:
        for _ in range(chunk):
            step(n)
            n += 1
        ev = torch.cuda.Event()
        ev.record(stream)
        if prev is not None:
            prev.synchronize()  # the chunk before this one is done: 1-2 chunks stay queued
        prev = ev
        if time.perf_counter() >= t_end:
            break
    torch.cuda.synchronize(dev)
    return n, time.perf_counter() - t0


DUMP_LIMIT = 64_000_000  # bytes of arrays one --dump-outputs run may write
DUMP_SEED = 0x64756D70


def dump_sample(n, k):
    """The records a dump holds whole: records 0 and n - 1 and a seeded draw of
    k of the n, ascending (the same for every run with the same arguments)."""
    import numpy as np
    if n <= k:
        return np.arange(n, dtype=np.int64)
    pick = np.random.default_rng(DUMP_SEED).choice(n, size=k, replace=False)
    return np.unique(np.concatenate([[0, n - 1], pick])).astype(np.int64)


def record_checksums(torch, buf, starts, lengths, chunk_bytes=1 << 24):
    """Two checksums of every record of the device byte buffer `buf` (record i
    = buf[starts[i] : starts[i] + lengths[i]]; numpy int64 arrays, ascending,
    not overlapping): the sum of its bytes and the sum of (j + 1) x byte j, as
    an [n, 2] float64 array (exact: both stay below 2^53).  Computed on the
    device as prefix sums over about `chunk_bytes` of the buffer at a time;
    bytes between the records (slot padding nothing writes) are not read into
    either sum."""
    import numpy as np
    out = np.empty((len(starts), 2), dtype=np.float64)
    ends = starts + lengths
    zero = torch.zeros(1, dtype=torch.int64, device=buf.device)
    i = 0
    while i < len(starts):
        j = max(i + 1, int(np.searchsorted(ends, starts[i] + chunk_bytes, side="right")))
        lo, hi = int(starts[i]), int(ends[j - 1])
        seg = buf[lo:hi].to(torch.int64)
        pos = torch.arange(hi - lo, dtype=torch.int64, device=buf.device)
        c0 = torch.cat([zero, torch.cumsum(seg, 0)])
        c1 = torch.cat([zero, torch.cumsum(seg * pos, 0)])
        s = torch.from_numpy(starts[i:j] - lo).to(buf.device)
        e = torch.from_numpy(ends[i:j] - lo).to(buf.device)
        plain = c0[e] - c0[s]
        weighted = c1[e] - c1[s] - (s - 1) * plain
        out[i:j, 0] = plain.cpu().numpy()
        out[i:j, 1] = weighted.cpu().numpy()
        i = j
    return out


def write_dump(d, arrays):
    """Write each array as d/<name>.npy (float32 or float64), DUMP_LIMIT bytes at most in all."""
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT, f"--dump-outputs would write {total} bytes"
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(d, name + ".npy"), a)


class UniformWork:
    """One rank's uniform workload (C2, C3, C4, perf): keys, the rotating
    batch sets, the step (one duplex launch, or a seal then an open), the
    timed region and the after-timing checks."""

    def __init__(self, args, cfg, A, torch, dev, N, S, sh):
        self.args, self.A, self.torch, self.dev = args, A, torch, dev
        self.cipher, self.N, self.S, self.sh = cfg["cipher"], N, S, sh
        self.L = L = cfg["len"]
        self.in_stride, self.out_stride = stride(L, args.align), stride(L + 16, args.align)
        self.stream = torch.cuda.current_stream(dev)
        sp = self.sp = self.stream.cuda_stream
        cipher = self.cipher
        # keys: SplitMix64 words of seed 0x6B6579 at 4*(global key id)
        raw = torch.empty(len(sh["key_ids"]) * 32, dtype=torch.uint8, device=dev)
        for i, kid in enumerate(sh["key_ids"]):
            assert A.dev_fill_splitmix(raw[32 * i:].data_ptr(), 32, SEED_KEY, 4 * kid, sp) == 0
        self.ctx = torch.empty(len(sh["key_ids"]) * A.dev_ctx_bytes(cipher), dtype=torch.uint8, device=dev)
        assert A.dev_prepare(cipher, raw.data_ptr(), len(sh["key_ids"]), self.ctx.data_ptr(), sp) == 0
        self.nonce = torch.tensor(sh["nonce_base"], dtype=torch.int64, device=dev)
        self.AD = AD = cfg.get("ad", 0)
        self.ad_buf = None
        if AD:
            self.ad_buf = torch.empty(N * AD, dtype=torch.uint8, device=dev)
            assert A.dev_fill_splitmix(self.ad_buf.data_ptr(), self.ad_buf.numel(), 0x6164,
                                       sh["first"] * AD // 8, sp) == 0
        self.ad_kw = dict(ad=self.ad_buf.data_ptr() if AD else 0, ad_stride=AD, ad_len=AD)
        self.sets = []
        for b in range(args.sets):
            pt = torch.empty(N * self.in_stride, dtype=torch.uint8, device=dev)
            # plaintext word w of the global stream = splitmix64(seed_pt + w)
            word0 = (sh["first"] * self.in_stride + b * (1 << 40)) // 8
            assert A.dev_fill_splitmix(pt.data_ptr(), pt.numel(), SEED_PT, word0, sp) == 0
            ct = torch.empty(N * self.out_stride, dtype=torch.uint8, device=dev)
            back = torch.empty(N * self.in_stride, dtype=torch.uint8, device=dev)
            st = torch.full((N,), 0xFF, dtype=torch.uint8, device=dev)
            self.sets.append((pt, ct, back, st))
        torch.cuda.synchronize(dev)
        self.sflags = A.FLAG_CT_GHASH if args.ct_ghash else 0
        # open order: verify first (the library's default since round 6; AES-GCM
        # always), or the opt-in one pass for ChaChaPoly
        self.vf = not args.one_pass or cipher == AES
        self.oflags = self.sflags | (A.FLAG_ONE_PASS if args.one_pass else 0)
        # Each step seals set b = s % sets and opens set (s - LAG) % sets, sealed
        # LAG steps earlier: the ciphertext an open reads was written two full
        # steps (> 700 MB of traffic) before, so it comes from HBM, not from the
        # 256 MiB Infinity Cache.  Every set is sealed once before timing, so
        # every open has ciphertext; a set's ciphertext is the same at every seal.
        self.lag = 2 if args.sets >= 3 else 0
        self.duplex = args.mode == "duplex"
        # --mode seal: encrypt only, one standalone seal launch per step
        self.seal_only = args.mode == "seal"
        self.dirs = 1 if self.seal_only else 2
        # lanes 0 in the jobs: the library's own choice, which differs
        # between a duplex launch and standalone seals/opens; self.lanes is
        # the duplex (timed) launch's, for the kernel names
        self.job_lanes = args.lanes
        self.lanes = args.lanes or (A.dev_duplex_lanes(cipher, N) if self.duplex else
                                    A.dev_default_lanes(cipher, N))
        self.per_step = args.events == "step"
        # --streams 2 (separate mode): consecutive steps (independent batch
        # sets) alternate between two streams, so step s+1's seal can start on
        # CUs that step s's open is leaving.  Set b is reused every `sets` steps.
        # With duplex steps the same alternation lets step s+1's launch fill
        # the CUs step s's tail leaves (steps s and s+1 touch disjoint sets;
        # steps s and s+2 share a stream, so the open of the set step s
        # sealed stays ordered after it).
        self.streams = [self.stream] + ([torch.cuda.Stream(dev)] if args.streams == 2 else [])
        self.opened = set()
        self._jobs = {}

    def _common(self):
        return dict(ctx=self.ctx.data_ptr(), nonce_base=self.nonce.data_ptr(), length=self.L,
                    n_records=self.N, recs_per_state=self.sh["rps"], lanes=self.job_lanes, **self.ad_kw)

    def seal(self, b, pt=None, ct=None, stream=None):
        if pt is None:
            pt, ct, _, _ = self.sets[b]
        return self.A.dev_uniform(False, self.cipher, inp=pt.data_ptr(), out=ct.data_ptr(),
                                  in_stride=self.in_stride, out_stride=self.out_stride,
                                  flags=self.sflags, stream=stream or self.sp, **self._common())

    def open_(self, b, stream=None):
        _, ct, back, st = self.sets[b]
        self.opened.add(b)
        return self.A.dev_uniform(True, self.cipher, inp=ct.data_ptr(), out=back.data_ptr(),
                                  in_stride=self.out_stride, out_stride=self.in_stride,
                                  status=st.data_ptr(), flags=self.oflags,
                                  stream=stream or self.sp, **self._common())

    def step_duplex(self, b, bo, stream=None):
        A = self.A
        self.opened.add(bo)
        jobs = self._jobs.get((b, bo))
        if jobs is None:  # built once per set pair: no Python struct work between launches
            pt, ct, _, _ = self.sets[b]
            _, cto, back, st = self.sets[bo]
            sj = A.uniform_job(inp=pt.data_ptr(), out=ct.data_ptr(), in_stride=self.in_stride,
                               out_stride=self.out_stride, flags=self.sflags, **self._common())
            oj = A.uniform_job(inp=cto.data_ptr(), out=back.data_ptr(), in_stride=self.out_stride,
                               out_stride=self.in_stride, status=st.data_ptr(), flags=self.oflags,
                               **self._common())
            jobs = self._jobs[(b, bo)] = (sj, oj)
        return A.dev_duplex(self.cipher, jobs[0], jobs[1], stream or self.sp)

    def untimed_step(self, w):
        """Step w outside the timed region (settle, warmup): the same launches."""
        b, bo = w % self.args.sets, (w - self.lag) % self.args.sets
        if self.duplex:
            assert self.step_duplex(b, bo) == 0
        elif self.seal_only:
            assert self.seal(b) == 0
        else:
            assert self.seal(b) == 0
            assert self.open_(bo) == 0

    def timed(self, steps, warmup, dist):
        """Settle (see settle()), warm up, then time exactly `steps` steps between barrier +
        synchronize on both sides; returns this rank's seconds.  Also sets
        launch_ms (HIP events on the launch stream)."""
        torch, dev, sets = self.torch, self.dev, self.args.sets
        for b in range(sets):
            assert self.seal(b) == 0
        self.settle_steps, self.settle_s = settle(torch, dev, self.stream, self.args.settle_ms,
                                                  self.untimed_step)
        for w in range(warmup):
            self.untimed_step(w)
        # Only the timed launches may leave what verify() checks: set 0's
        # sealed records are zeroed (timed step 0 seals set 0 again, step 2
        # opens it), every open output is zeroed and every status set to
        # 0xFF, and only sets opened from here on are checked.
        self.sets[0][1].zero_()
        for _, _, back, st in self.sets:
            back.zero_()
            st.fill_(0xFF)
        self.opened = set()
        torch.cuda.synchronize(dev)
        if dist:
            dist.barrier()
        per_step = self.per_step
        if self.duplex or not per_step:  # launch boundaries (duplex) or just the region's ends
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        else:
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True),
                   torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if self.duplex or not per_step:
            ev[0].record(self.stream)
        for s in range(steps):
            b, bo = s % sets, (s - self.lag) % sets
            if self.duplex or not per_step:
                if self.duplex:
                    rc = self.step_duplex(b, bo, self.streams[s % len(self.streams)].cuda_stream)
                elif self.seal_only:
                    rc = self.seal(b, stream=self.streams[s % len(self.streams)].cuda_stream)
                else:
                    st_ = self.streams[s % len(self.streams)].cuda_stream
                    rc = self.seal(b, stream=st_) or self.open_(bo, stream=st_)
                if per_step or s == steps - 1 or (s == 0 and steps > 1):
                    for other in self.streams[1:]:  # the end event covers every stream's steps
                        self.stream.wait_stream(other)
                    ev[s + 1].record(self.stream)
                if rc:
                    raise RuntimeError(f"launch failed {rc:#x}")
                continue
            st_ = self.streams[s % len(self.streams)]
            ev[s][0].record(st_)
            rc1 = self.seal(b, stream=st_.cuda_stream)
            ev[s][1].record(st_)
            rc2 = self.open_(bo, stream=st_.cuda_stream)
            ev[s][2].record(st_)
            if rc1 or rc2:
                raise RuntimeError(f"launch failed {rc1:#x} {rc2:#x}")
        torch.cuda.synchronize(dev)
        elapsed = time.perf_counter() - t0
        self.ev = ev
        if self.duplex or not per_step:
            # average launch interval over the timed region, gaps included,
            # from the end of step 1 on: the first step also carries the
            # host's submission of the first launch after ev[0] (~3 us per
            # step at K = 20), which is no kernel time
            per = 1 if (self.duplex or self.seal_only) else 2  # launches per step
            if steps > 1:
                self.launch_ms = ev[1].elapsed_time(ev[steps]) / (steps - 1) / per
            else:
                self.launch_ms = ev[0].elapsed_time(ev[steps]) / steps / per
        else:
            self.launch_ms = None
        return elapsed

    def per_direction_ms(self):
        """Seal / open launch times: per-step events, or (duplex, ends, two
        streams, seal mode) a separate serial pass of the two kernels, run
        right after the timed region (the settled clock) into scratch outputs:
        the sets' sealed records and opened outputs stay those of the timed
        launches, which verify() checks.  The opens read the sets' sealed
        records (every set is sealed before timing)."""
        torch, steps, A = self.torch, self.args.steps, self.A
        if not (self.duplex or not self.per_step or len(self.streams) > 1 or self.seal_only):
            seal_ms = sum(e[0].elapsed_time(e[1]) for e in self.ev) / steps
            open_ms = sum(e[1].elapsed_time(e[2]) for e in self.ev) / steps
            return seal_ms, open_ms
        N = self.N
        ct_s = torch.empty(N * self.out_stride, dtype=torch.uint8, device=self.dev)
        back_s = torch.empty(N * self.in_stride, dtype=torch.uint8, device=self.dev)
        st_s = torch.empty(N, dtype=torch.uint8, device=self.dev)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        reps, sets = 20, self.args.sets
        e[0].record(self.stream)
        # seal mode: the timed launches ARE the seal pass (and a profile's
        # last --steps dispatches of the seal kernel stay the timed ones)
        for r in range(0 if self.seal_only else reps):
            pt = self.sets[r % sets][0]
            assert self.seal(None, pt=pt, ct=ct_s) == 0
        e[1].record(self.stream)
        for r in range(reps):
            ct = self.sets[(r - self.lag) % sets][1]  # every set holds valid CT after the timed steps
            assert A.dev_uniform(True, self.cipher, inp=ct.data_ptr(), out=back_s.data_ptr(),
                                 in_stride=self.out_stride, out_stride=self.in_stride,
                                 status=st_s.data_ptr(), flags=self.oflags, stream=self.sp,
                                 **self._common()) == 0
        e[2].record(self.stream)
        torch.cuda.synchronize(self.dev)
        del ct_s, back_s, st_s
        seal_ms = self.launch_ms if self.seal_only else e[0].elapsed_time(e[1]) / reps
        return seal_ms, e[1].elapsed_time(e[2]) / reps

    def dump(self, d):
        """--dump-outputs: what the last timed step left for its caller — the
        records it sealed (ciphertext + tag), the records it opened and the
        opens' statuses — as float arrays under d: each byte as one float32,
        whole for a fixed seeded sample of the records (sample_records: their
        indices), and two float64 checksums of every record of the batch
        (record_checksums), so that every output byte bears on the dump."""
        import numpy as np
        torch, N, L = self.torch, self.N, self.L
        torch.cuda.synchronize(self.dev)
        last = self.args.steps - 1
        sealed = self.sets[last % self.args.sets][1]
        _, _, opened, status = self.sets[(last - self.lag) % self.args.sets]
        idx = dump_sample(N, 1024)
        idx_d = torch.from_numpy(idx).to(self.dev)
        rec = np.arange(N, dtype=np.int64)

        def whole(buf, stride_, n):
            return buf.view(N, stride_)[idx_d, :n].cpu().numpy().astype(np.float32)

        arrays = {"sample_records": idx.astype(np.float64),
                  "sealed_sample": whole(sealed, self.out_stride, L + 16),
                  "sealed_checksums": record_checksums(torch, sealed, rec * self.out_stride,
                                                       np.full(N, L + 16, dtype=np.int64))}
        if not self.seal_only:
            arrays["opened_sample"] = whole(opened, self.in_stride, L)
            arrays["opened_checksums"] = record_checksums(torch, opened, rec * self.in_stride,
                                                          np.full(N, L, dtype=np.int64))
            arrays["open_status"] = status.cpu().numpy().astype(np.float32)
        write_dump(d, arrays)

    def verify(self, config, rank, world):
        """After the timed region: every opened set's statuses are 0 and its
        opened records equal its plaintext; set 0's sealed records (written by
        the timed kernels) hash to the golden digest of this rank's shard."""
        import hashlib
        torch, N, L = self.torch, self.N, self.L
        torch.cuda.synchronize(self.dev)
        st_ok = rt_ok = True
        for b in sorted(self.opened):
            pt, _, back, st = self.sets[b]
            st_ok &= bool((st == 0).all().item())
            rt_ok &= bool(torch.equal(back.view(N, self.in_stride)[:, :L], pt.view(N, self.in_stride)[:, :L]))
        strong = bool(CONFIGS[config].get("strong"))
        want = shard_golden(config, rank, world, strong)
        # the golden plaintext is the SplitMix64 stream over roundup16(len)
        # slots (tests/golden/gen_shard_digests.py): other slot widths differ
        if want is not None and self.in_stride == stride(L, 16):
            ct = self.sets[0][1].view(N, self.out_stride)[:, :L + 16].contiguous().cpu().numpy()
            got = hashlib.sha256(ct.tobytes()).hexdigest()
            digest = "match" if got == want else "MISMATCH"
        else:
            digest = "no golden for this rank/layout"
        ok = st_ok and rt_ok and digest != "MISMATCH"
        return {"ok": ok, "sets_opened": len(self.opened), "statuses_zero": st_ok,
                "round_trip": rt_ok, "sealed_digest_set0": digest,
                "golden": "tests/golden/shard_digests.json"}


def n1_reference(args, cfg, A, torch, dev, rank, dist, wl, N, S, world):
    """The N = 1 value of this config measured in the same run: rank 0 runs
    the per-GPU work alone — its own shard for weak scaling, the whole job
    (world x its shard) for strong scaling — while the other ranks wait at a
    barrier.  per_gpu_efficiency = value / (N x this)."""
    dist.barrier()
    v = 0.0
    if rank == 0:
        if cfg.get("strong"):
            w1 = UniformWork(args, cfg, A, torch, dev, N * world, S * world,
                             shard(N * world, S * world, 0, 1))
            el = w1.timed(args.steps, args.warmup, None)
            v = w1.dirs * N * world * w1.L * args.steps / el / GIB
            del w1
        else:
            el = wl.timed(args.steps, args.warmup, None)
            v = wl.dirs * N * wl.L * args.steps / el / GIB
    v = max_over_ranks(dist, torch, dev, v)
    dist.barrier()
    return round(v, 2)


def verify_over_ranks(dist, torch, dev, verify):
    """Every rank checks its own shard (statuses, round trip, the golden
    digest of its set-0 output); with a process group the line's `verified`
    is all ranks' verdict and `verify.ranks` lists each rank's (ok, digest:
    1 match, 0 no golden for that rank/layout, -1 MISMATCH)."""
    if dist is None or verify is None:
        return verify
    d = verify.get("sealed_digest_set0", verify.get("sealed_digest"))
    code = 1 if d == "match" else -1 if d == "MISMATCH" else 0
    mine = cpu_if_rehearsal(torch.tensor([1 if verify["ok"] else 0, code], dtype=torch.int64, device=dev))
    got = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
    dist.all_gather(got, mine)
    ranks = [{"ok": bool(g[0].item()), "digest": {1: "match", 0: "no golden", -1: "MISMATCH"}[int(g[1].item())]}
             for g in got]
    verify["rank0_ok"] = verify["ok"]
    verify["ok"] = all(r["ok"] for r in ranks)
    verify["ranks"] = ranks
    return verify


def finish(args, result, rank, world, dist):
    """Per-GPU efficiency when an N = 1 value is given, the
    rehearsal label, then rank 0 prints the one JSON line."""
    n1 = args.n1_value or result.get("n1_in_run")
    if n1 and world > 1:
        # (aggregate GiB/s at N) / (N x GiB/s at N = 1), for weak and strong
        # scaling alike (strong: total work fixed, so this is speedup / N)
        result["per_gpu_efficiency"] = round(result["value"] / (world * n1), 4)
        result["n1_value"] = n1
        result["n1_source"] = ("--n1-value" if args.n1_value else
                               "in-run: rank 0 alone on the same per-GPU work, other ranks at a barrier")
    if dist is not None:
        result["process_group"] = {"backend": str(dist.get_backend()), "world_size": dist.get_world_size()}
    if REHEARSE and world > 1:
        # every rank on one GPU, collectives on gloo: exercises the N > 1 code
        # path only; per-kernel rates of ranks sharing a GPU mean nothing
        result.pop("roofline", None)
        result["rehearsal"] = (f"{world} ranks on ONE GPU, gloo process group (collectives via host "
                               "memory): a code-path rehearsal, not a multi-GPU measurement")
    if rank == 0:
        emit_line(result)
    if dist:
        dist.destroy_process_group()


def xfer_leg(args, torch, dist, dev, A, rank, world, N, L, in_stride, out_stride, sh, sets, seal):
    """the batch starts and ends on rank 0's GPU.  Rank 0 holds
    the whole job's plaintext (world shards, each equal to that rank's set-0
    input), RCCL scatters the shards, every rank seals its own, RCCL gathers
    the sealed shards back to rank 0.  Timed per phase (max over ranks);
    reported beside, never instead of, the device-resident value."""
    from distribute import scatter_records, gather_records
    sp = torch.cuda.current_stream(dev).cuda_stream
    shard_in, shard_out = N * in_stride, N * out_stride
    full_in = full_out = None
    if rank == 0:
        full_in = torch.empty(world * shard_in, dtype=torch.uint8, device=dev)
        full_out = torch.empty(world * shard_out, dtype=torch.uint8, device=dev)
        for g in range(world):  # shard g = rank g's set-0 plaintext (same SplitMix64 words)
            assert A.dev_fill_splitmix(full_in[g * shard_in:].data_ptr(), shard_in, 0x7074,
                                       (g * N * in_stride) // 8, sp) == 0
    local_in = torch.empty(shard_in, dtype=torch.uint8, device=dev)
    local_out = torch.empty(shard_out, dtype=torch.uint8, device=dev)
    phases = []
    for rep in range(args.xfer_reps + 1):
        torch.cuda.synchronize(dev)
        dist.barrier()
        t0 = time.perf_counter()
        if REHEARSE:  # gloo scatters CPU tensors
            tmp = torch.empty(shard_in, dtype=torch.uint8)
            scatter_records(tmp, full_in.cpu() if rank == 0 else None, src=0)
            local_in.copy_(tmp)
        else:
            scatter_records(local_in, full_in, src=0)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        if seal(0, local_in, local_out):
            raise RuntimeError("seal launch failed")
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        if REHEARSE:
            tmp = torch.empty(world * shard_out, dtype=torch.uint8) if rank == 0 else None
            gather_records(local_out.cpu(), tmp, dst=0)
            if rank == 0:
                full_out.copy_(tmp)
        else:
            gather_records(local_out, full_out, dst=0)
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        if rep:  # rep 0 warms RCCL's channels
            phases.append((t1 - t0, t2 - t1, t3 - t2, t3 - t0))
    ph = cpu_if_rehearsal(torch.tensor(phases, dtype=torch.float64, device=dev).mean(0))
    dist.all_reduce(ph, op=dist.ReduceOp.MAX)
    # checks: scattered shard == this rank's own input; gathered shard g ==
    # rank g's sealed output (int64 checksums, all_gathered)
    ok = cpu_if_rehearsal(torch.tensor([1 if torch.equal(local_in, sets[0][0]) else 0], device=dev))
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    mine = cpu_if_rehearsal(local_out.view(torch.int64).sum().reshape(1))
    sums = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(sums, mine)
    good = bool(ok.item())
    if rank == 0:
        for g in range(world):
            got = full_out[g * shard_out:(g + 1) * shard_out].view(torch.int64).sum()
            good &= bool(got.item() == sums[g].item())
    sc, se, ga, tot = (float(x) * 1e3 for x in ph.tolist())
    return {"collective": ("torch.distributed scatter/gather on gloo via host memory (one-GPU rehearsal)"
                           if REHEARSE else
                           "torch.distributed scatter/gather on nccl (RCCL grouped send/recv over xGMI)"),
            "src_dst_rank": 0, "shard_in_bytes": shard_in, "shard_out_bytes": shard_out,
            "scatter_ms": round(sc, 4), "seal_ms": round(se, 4), "gather_ms": round(ga, 4),
            "total_ms": round(tot, 4),
            "seal_gibs_incl_xfer": round(N * L * world / (tot * 1e-3) / GIB, 2),
            "scatter_gbs": round((world - 1) * shard_in / (sc * 1e-3) / 1e9, 1),
            "gather_gbs": round((world - 1) * shard_out / (ga * 1e-3) / 1e9, 1),
            "verified": good, "reps": args.xfer_reps}


def run_mixed(args, cfg, A, torch, dev, rank, world, dist):
    """C5: mixed-cipher ragged batch, seal then open (tags verified)."""
    import numpy as np
    R, S = cfg["records"], cfg["states"]
    lay = mixed_layout(R, S, rank)
    sp = torch.cuda.current_stream(dev).cuda_stream
    rec_dt = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("nonce", "<u8"), ("ctx_off", "<u8"),
                       ("ad_off", "<u8"), ("len", "<u4"), ("ad_len", "<u4")])
    assert rec_dt.itemsize == 48
    pt = torch.empty(lay["total"], dtype=torch.uint8, device=dev)
    assert A.dev_fill_splitmix(pt.data_ptr(), pt.numel(), SEED_PT, rank << 40, sp) == 0
    ct = torch.empty_like(pt)
    back = torch.empty_like(pt)
    groups = []
    for cipher, parity in ((CHACHA, 0), (AES, 1)):
        states = [s for s in range(S) if (rank * S + s) % 2 == parity]
        if not states:
            continue
        cb = A.dev_ctx_bytes(cipher)
        raw = torch.empty(len(states) * 32, dtype=torch.uint8, device=dev)
        for i, s in enumerate(states):
            assert A.dev_fill_splitmix(raw[32 * i:].data_ptr(), 32, SEED_KEY, 4 * (rank * S + s), sp) == 0
        ctx = torch.empty(len(states) * cb, dtype=torch.uint8, device=dev)
        assert A.dev_prepare(cipher, raw.data_ptr(), len(states), ctx.data_ptr(), sp) == 0
        slot_of = {s: i for i, s in enumerate(states)}
        idx = np.nonzero((lay["st_global"] % 2) == parity)[0]
        recs = np.zeros(len(idx), dtype=rec_dt)
        recs["in_off"] = lay["off"][idx]
        recs["out_off"] = lay["off"][idx]
        recs["nonce"] = lay["nonce"][idx]
        recs["ctx_off"] = np.array([slot_of[s] for s in lay["st_local"][idx]], dtype=np.uint64) * cb
        recs["len"] = lay["lens"][idx]
        d_recs = torch.from_numpy(recs.view(np.uint8)).to(dev)
        st = torch.empty(len(idx), dtype=torch.uint8, device=dev)
        groups.append(dict(cipher=cipher, ctx=ctx, recs=d_recs, n=len(idx), st=st, idx=idx,
                           bytes=int(lay["lens"][idx].sum()), states=len(states)))
    torch.cuda.synchronize(dev)

    oflags = A.FLAG_ONE_PASS if args.one_pass else 0  # verify-first unless --one-pass

    def launch(g, open_, stream=sp, inp=None, out=None):
        inp = inp if inp is not None else (ct if open_ else pt)
        out = out if out is not None else (back if open_ else ct)
        return A.dev_ragged(open_, g["cipher"], ctx_base=g["ctx"].data_ptr(),
                            recs=g["recs"].data_ptr(), inp=inp.data_ptr(),
                            out=out.data_ptr(), n_records=g["n"],
                            status=g["st"].data_ptr() if open_ else 0, lanes=args.lanes,
                            flags=A.FLAG_FAST | (oflags if open_ else 0), stream=stream)

    # Two streams: the LDS-bound AES-GCM kernel and the VALU-bound ChaChaPoly
    # kernel share the CUs instead of running back to back (fork/join by
    # events, no host sync).  --c5-join step (default): each cipher's open
    # depends only on its own seal, as the records do, so one half's open
    # fills the CUs the other half's seal leaves in its tail; the halves
    # join at the end of the step.  phase: both seals finish before either
    # open (round 4's shape).
    main_s = torch.cuda.current_stream(dev)
    side = (C5_STREAMS[1] if C5_STREAMS and args.c5_prio != "aes" else
            torch.cuda.Stream(dev, priority=-1 if args.c5_prio == "aes" else 0)) \
        if args.c5_streams == 2 and len(groups) == 2 else None  # the AES-GCM half
    cha_s = torch.cuda.Stream(dev, priority=-1) if side is not None and args.c5_prio == "chacha" else None
    fork = [torch.cuda.Event() for _ in range(2)]
    join = [torch.cuda.Event() for _ in range(2)]

    # --c5-sets 2: ciphertext sets alternate; step k seals into cts[k % 2]
    # and opens cts[(k + 1) % 2], sealed by step k - 1 (the same records
    # and nonces, so the same bytes): the step's four launches are
    # independent and run on four streams
    cts = [ct, torch.empty_like(pt)] if args.c5_sets == 2 and side is not None else None
    sides2 = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)] if cts else None
    kstep = [0]
    if cts:
        for g in groups:
            assert launch(g, False, inp=pt, out=cts[1]) == 0
        torch.cuda.synchronize(dev)

    def step():
        if cts:
            k = kstep[0]
            kstep[0] += 1
            sealed, opened = cts[k % 2], cts[(k + 1) % 2]
            fork[0].record(main_s)
            for st_ in (side, *sides2):
                st_.wait_event(fork[0])
            rc = launch(groups[1], False, side.cuda_stream, inp=pt, out=sealed) \
                or launch(groups[1], True, sides2[0].cuda_stream, inp=opened, out=back) \
                or launch(groups[0], False, main_s.cuda_stream, inp=pt, out=sealed) \
                or launch(groups[0], True, sides2[1].cuda_stream, inp=opened, out=back)
            if rc:
                raise RuntimeError(f"launch failed {rc:#x}")
            for i, st_ in enumerate((side, *sides2)):
                ev = join[0] if i == 0 else torch.cuda.Event()
                ev.record(st_)
                main_s.wait_event(ev)
            return
        if side is not None and args.c5_join == "step":
            fork[0].record(main_s)
            side.wait_event(fork[0])
            cs = main_s
            if cha_s is not None:
                cha_s.wait_event(fork[0])
                cs = cha_s
            if args.c5_first == "chacha":
                rc = launch(groups[0], False, cs.cuda_stream) or launch(groups[0], True, cs.cuda_stream) \
                    or launch(groups[1], False, side.cuda_stream) or launch(groups[1], True, side.cuda_stream)
            else:
                rc = launch(groups[1], False, side.cuda_stream) or launch(groups[0], False, cs.cuda_stream) \
                    or launch(groups[1], True, side.cuda_stream) or launch(groups[0], True, cs.cuda_stream)
            if rc:
                raise RuntimeError(f"launch failed {rc:#x}")
            join[0].record(side)
            main_s.wait_event(join[0])
            if cha_s is not None:
                join[1].record(cha_s)
                main_s.wait_event(join[1])
            return
        for open_ in (False, True):
            if side is None:
                for g in groups:
                    rc = launch(g, open_)
                    if rc:
                        raise RuntimeError(f"launch failed {rc:#x}")
                continue
            fork[open_].record(main_s)
            side.wait_event(fork[open_])
            rc = launch(groups[1], open_, side.cuda_stream) or launch(groups[0], open_)
            if rc:
                raise RuntimeError(f"launch failed {rc:#x}")
            join[open_].record(side)
            main_s.wait_event(join[open_])

    settled = [0, 0.0]

    def timed(d):
        settled[:] = settle(torch, dev, torch.cuda.current_stream(dev), args.settle_ms,
                            lambda n: step())
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize(dev)
        if d:
            d.barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    elapsed = max_over_ranks(dist, torch, dev, timed(dist))
    if dist:
        dist.barrier()
    if cts:  # verify the set the last timed step sealed
        ct = cts[(kstep[0] - 1) % 2]
    if args.dump_outputs:
        dump_mixed(dump_dir(args, rank, world), torch, dev, lay, groups, ct, back)
    # per-kernel times (separate, untimed pass) for the roofline line
    per = []
    for open_ in (False, True) if args.full else ():
        for g in groups:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                launch(g, open_)
            e1.record()
            torch.cuda.synchronize(dev)
            per.append((e0.elapsed_time(e1) / 5, g, open_))
    ok = args.full and all(bool((g["st"] == 0).all().item()) for g in groups)
    verify = None
    if args.full and not args.no_verify:
        # every record's round trip (a device compare of the whole plaintext
        # area: the slots' padding is never written by the opens, so compare
        # record bytes only, as a masked view), and the sealed records of the
        # timed kernels against the golden digest of this rank's shard
        import hashlib
        starts = torch.from_numpy(lay["off"]).to(dev)
        lens_t = torch.from_numpy(lay["lens"]).to(dev)
        cov = torch.zeros(lay["total"] + 1, dtype=torch.int32, device=dev)
        cov.index_add_(0, starts, torch.ones_like(starts, dtype=torch.int32))
        cov.index_add_(0, starts + lens_t, -torch.ones_like(starts, dtype=torch.int32))
        mask = torch.cumsum(cov, 0, dtype=torch.int32)[:-1] > 0
        rt_ok = bool(torch.equal(back[mask], pt[mask]))
        del mask, cov
        want = shard_golden(args.config, rank, world, False)
        digest = "no golden for this rank"
        if want is not None:
            h = hashlib.sha256()
            ct_h = ct.cpu().numpy()
            for o, n in zip(lay["off"].tolist(), lay["lens"].tolist()):
                h.update(ct_h[o:o + n + 16])
            digest = "match" if h.hexdigest() == want else "MISMATCH"
            del ct_h
        verify = {"ok": ok and rt_ok and digest != "MISMATCH", "statuses_zero": ok, "round_trip": rt_ok,
                  "sealed_digest": digest, "golden": "tests/golden/shard_digests.json"}
    verify = verify_over_ranks(dist, torch, dev, verify)
    payload = sum(g["bytes"] for g in groups)
    value = 2.0 * payload * world * args.steps / elapsed / GIB
    result = {
        "metric": "GiB/s device-resident AEAD encrypt+decrypt, mixed 64B-16KiB records per GPU",
        "value": round(value, 2), "unit": "GiB/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(elapsed * 1e3 / args.steps, 4),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u32",
        "data": "synthetic (SplitMix64 lengths, plaintext and keys, SURVEY.md 8d C5), resident in HBM",
        "config": {"workload": cfg["workload"], "config": args.config, "records_per_gpu": R,
                   "states_per_gpu": S, "payload_bytes_per_step": int(2 * payload * world),
                   "streams": 2 if side is not None else 1,
                   "join": args.c5_join if side is not None else None,
                   "sets": 2 if cts else 1,
                   "parallelism": f"states x{world}",
                   "settle": {"ms": args.settle_ms, "steps": settled[0], "s": round(settled[1], 3)}},
        "open_order": ("ChaChaPoly one pass (NOISE_AEAD_FLAG_ONE_PASS), AES-GCM verify-first"
                       if args.one_pass else "verify-first (the default, both ciphers)"),
    }
    if not args.full:
        return finish(args, result, rank, world, dist)
    ms, g, open_ = max(per, key=lambda x: x[0])
    alg = 2 * g["bytes"] + 16 * g["n"] + 40 * g["states"]
    achieved = alg / (ms * 1e-3) / 1e9
    # the kernel the library dispatches (aead_api.hip run_ragged), as rocprofv3 names it
    if g["cipher"] == CHACHA and not args.lanes and os.environ.get("NOISE_AEAD_SEG", "1") != "0" \
            and g["n"] >= 16384:  # run_ragged: the segmented one-lane kernel (chachapoly_seg.hip)
        kname = f"chachapoly_seg_ragged<{'true' if open_ else 'false'}>"
    elif g["cipher"] == CHACHA:  # run_ragged: 8 lanes below 128 Ki records, else 4
        k = args.lanes or (8 if g["n"] < 131072 else 4)
        kname = (f"chachapoly_open_ragged<{k}, true, {'false' if args.one_pass else 'true'}>"
                 if open_ else f"chachapoly_seal_ragged<{k}, true>")
    else:  # gcm_ragged_shape: (threads, records per group, lanes per record) by batch size
        n_aes = g["n"]
        wg, r, kl = (1024, 2, 4) if n_aes >= 131072 else ((1024, 2, 8) if n_aes >= 65536 else (256, 1, 4))
        kname = f"gcm_ragged_staged<{'true' if open_ else 'false'}, true, {wg}, false, {r}, {kl}>"
    pmc = load_pmc(args.config, kname)
    result.update({
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                     "traffic": pmc.get("hbm_bytes_per_launch"),
                     "kernel": kname, "algorithmic_bytes_per_launch": alg,
                     "avg_launch_ms": round(ms, 5), "issue_bound": issue_bound(pmc, ms)},
        "kernels_ms": {(("chacha" if gg["cipher"] == CHACHA else "aes") + ("_open" if o else "_seal")): round(m, 4)
                       for m, gg, o in per},
        "all_tags_verified": ok,
    })
    if verify is not None:
        result["verified"] = verify.pop("ok")
        result["verify"] = verify
    if dist is not None and not args.no_xfer:
        try:  # reported beside the value; a failure here never voids the bench line
            result["scatter_gather"] = xfer_leg_mixed(args, torch, dist, dev, A, rank, world, R, S,
                                                      lay, pt, groups, launch)
        except Exception as e:
            result["scatter_gather"] = {"error": repr(e)}
        # a failed scatter/gather is stated at the top level of
        # the line (it still never voids the GPU number)
        sgr = result["scatter_gather"]
        result["scatter_gather_ok"] = "error" not in sgr and bool(sgr.get("verified", sgr.get("ok", False)))
    if world > 1 and not args.no_n1 and args.n1_value is None:
        dist.barrier()  # rank 0 alone on its own shard: the in-run N = 1 value
        v = 2.0 * payload * args.steps / timed(None) / GIB if rank == 0 else 0.0
        result["n1_in_run"] = round(max_over_ranks(dist, torch, dev, v), 2)
        dist.barrier()
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            result["cpu_baseline"] = cpu_baseline_mixed()
        except Exception as e:  # reported, never fatal to the GPU number
            result["cpu_baseline"] = {"error": str(e)}
    finish(args, result, rank, world, dist)


def dump_mixed(d, torch, dev, lay, groups, ct, back):
    """--dump-outputs of C5: as UniformWork.dump, for the ragged batch.  The
    sampled records' bytes lie end to end in sealed_sample (len + 16 each) and
    opened_sample (len each); open_status is in record order."""
    import numpy as np
    torch.cuda.synchronize(dev)
    off, lens = lay["off"], lay["lens"]
    idx = dump_sample(len(lens), 256)

    def whole(buf, extra):
        at = np.concatenate([np.arange(off[i], off[i] + lens[i] + extra) for i in idx])
        return buf[torch.from_numpy(at).to(dev)].cpu().numpy().astype(np.float32)

    status = np.empty(len(lens), dtype=np.float32)
    for g in groups:
        status[g["idx"]] = g["st"].cpu().numpy()
    write_dump(d, {"sample_records": idx.astype(np.float64),
                   "sealed_sample": whole(ct, 16),
                   "sealed_checksums": record_checksums(torch, ct, off, lens + 16),
                   "opened_sample": whole(back, 0),
                   "opened_checksums": record_checksums(torch, back, off, lens),
                   "open_status": status})


def cpu_baseline_mixed(budget_s: float = 12.0):
    """C5's CPU row: the reference's CipherState API (oracle/_ref/ref_bench
    mixed) over the C5 length mix (64 B-16 KiB, ChaChaPoly / AESGCM by state
    parity), encrypt then decrypt+verify, one thread per physical core of
    this job's CPU share."""
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_bench")
    kind = "reference"
    if not os.path.exists(ref):
        ref, kind = os.path.join(ROOT, "oracle", "_build", "port_bench"), "port"
    if not os.path.exists(ref):
        return None
    hc = host_cpu()
    phys = hc["physical_cores"] or hc["usable_cpus"]
    threads = max(1, min(phys, hc["usable_cpus"], hc["cpu_share"] or phys))
    probe = json.loads(subprocess.run([ref, "mixed", "x", "0", "600", "1"], capture_output=True,
                                      text=True, timeout=120, check=True).stdout)
    per_thread = max(600, int(600 * budget_s / max(probe["seconds"], 1e-6) / threads))
    r = json.loads(subprocess.run([ref, "mixed", "x", "0", str(per_thread), str(threads)],
                                  capture_output=True, text=True, timeout=600, check=True).stdout)
    return {"value": round(r["gib_per_s"], 4), "unit": "GiB/s", "cores": threads, "kind": kind,
            "single_thread": round(probe["gib_per_s"], 4), "ok": r["ok"],
            "sample": (f"{'noise-c ref backend CipherState API' if kind == 'reference' else 'oracle restatement'}"
                       f" over the C5 mix (64 B-16 KiB, ChaChaPoly even / AESGCM odd states of 256 "
                       f"records): {threads} threads x {per_thread} records, each encrypted then "
                       f"decrypted+verified, wall clock; 1 thread: {probe['gib_per_s']:.3f} GiB/s"),
            **hc}


def xfer_leg_mixed(args, torch, dist, dev, A, rank, world, R, S, lay, pt, groups, launch):
    """The C5 form of xfer_leg: rank 0 holds every rank's
    ragged plaintext shard, RCCL scatters them (shards differ in size: packed
    back to back, each rounded up to 64 B only, one point-to-point send per
    peer — distribute.scatter_records_v; VERDICT r5 weak 10: round 5 padded
    every shard to the largest's size), every rank seals its own
    records of both ciphers, RCCL gathers the sealed shards back.  The record
    descriptors are not sent: each rank derives its own from the shared layout
    rule (mixed_layout).  Timed per phase, max over ranks; verified."""
    from distribute import gather_records_v, scatter_records_v
    sp = torch.cuda.current_stream(dev).cuda_stream
    totals = [mixed_layout(R, S, g)["total"] for g in range(world)]
    sizes = [(t + 63) // 64 * 64 for t in totals]
    offs = [sum(sizes[:g]) for g in range(world)]
    full_in = full_out = None
    if rank == 0:
        full_in = torch.zeros(sum(sizes), dtype=torch.uint8, device=dev)
        full_out = torch.zeros(sum(sizes), dtype=torch.uint8, device=dev)
        for g in range(world):  # shard g = rank g's plaintext (its SplitMix64 words)
            assert A.dev_fill_splitmix(full_in[offs[g]:].data_ptr(), totals[g], SEED_PT, g << 40, sp) == 0
    local_in = torch.zeros(sizes[rank], dtype=torch.uint8, device=dev)
    local_out = torch.zeros(sizes[rank], dtype=torch.uint8, device=dev)
    phases = []
    for rep in range(args.xfer_reps + 1):
        torch.cuda.synchronize(dev)
        dist.barrier()
        t0 = time.perf_counter()
        if REHEARSE:
            tmp = torch.empty(sizes[rank], dtype=torch.uint8)
            scatter_records_v(tmp, full_in.cpu() if rank == 0 else None, sizes, src=0)
            local_in.copy_(tmp)
        else:
            scatter_records_v(local_in, full_in, sizes, src=0)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for g in groups:
            if launch(g, False, inp=local_in, out=local_out):
                raise RuntimeError("seal launch failed")
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        if REHEARSE:
            tmp = torch.empty(sum(sizes), dtype=torch.uint8) if rank == 0 else None
            gather_records_v(local_out.cpu(), tmp, sizes, dst=0)
            if rank == 0:
                full_out.copy_(tmp)
        else:
            gather_records_v(local_out, full_out, sizes, dst=0)
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        if rep:
            phases.append((t1 - t0, t2 - t1, t3 - t2, t3 - t0))
    ph = cpu_if_rehearsal(torch.tensor(phases, dtype=torch.float64, device=dev).mean(0))
    dist.all_reduce(ph, op=dist.ReduceOp.MAX)
    total = lay["total"]
    ok = cpu_if_rehearsal(torch.tensor([1 if torch.equal(local_in[:total], pt[:total]) else 0],
                                       device=dev))
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    mine = cpu_if_rehearsal(local_out.view(torch.int64).sum().reshape(1))
    sums = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(sums, mine)
    good = bool(ok.item())
    if rank == 0:
        for g in range(world):
            got = full_out[offs[g]:offs[g] + sizes[g]].view(torch.int64).sum()
            good &= bool(got.item() == sums[g].item())
    sc, se, ga, tot = (float(x) * 1e3 for x in ph.tolist())
    payload = sum(int(mixed_layout(R, S, g)["lens"].sum()) for g in range(world))
    return {"collective": ("torch.distributed batched send/recv on gloo via host memory (one-GPU rehearsal)"
                           if REHEARSE else
                           "torch.distributed batched send/recv on nccl (RCCL grouped send/recv over xGMI)"),
            "src_dst_rank": 0, "shard_bytes": totals, "sent_bytes": sizes,
            "scatter_ms": round(sc, 4), "seal_ms": round(se, 4), "gather_ms": round(ga, 4),
            "total_ms": round(tot, 4),
            "seal_gibs_incl_xfer": round(payload / (tot * 1e-3) / GIB, 2),
            "verified": good, "reps": args.xfer_reps}


if __name__ == "__main__":
    main()
