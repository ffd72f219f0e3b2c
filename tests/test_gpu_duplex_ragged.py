"""GPU parity of noise_aead_dev_duplex_ragged: one mixed batch sealed and another
opened per call.

The contract (include/noise_aead_hip.h): the result is exactly
noise_aead_dev_seal_ragged(seal_job) followed by
noise_aead_dev_open_ragged(open_job) — every byte of both outputs, both status
arrays, every byte the separate calls leave untouched.  Each case builds two
independent ragged jobs, X to seal and Y to open (Y's input sealed by the
oracle), runs the duplex call, runs the two separate calls on fresh copies of
the same buffers (outputs pre-filled with 0xA5), and asserts, in this order:

 1. aead.last_plan() names the expected kernel: one of the three shared
    kernels (gcm_duplex_ragged, chachapoly_seg_duplex,
    chachapoly_duplex_ragged), or a standalone one where the jobs cannot share;
 2. torch.equal on the whole seal output buffer, the whole open output buffer
    and both status arrays;
 3. the oracle: every sealed record and every opened plaintext (the cases of
    16 384 records or more: a seeded sample of 400 records per job, every
    record over 8 KiB, the first and the last).

Every Y job has every 37th record tampered (status 1; out of place its output
keeps 0xA5, in place CT || tag reads back as given) and one record of 65520
bytes (status 2, nothing written); every X job has one 65520-byte record and
its status array.  Half of Y's records are in place, half out of place, in one
batch.

The switches of kernel choice are read once per process, so the cases that
need NOISE_AEAD_RAGGED_DUPLEX set run this file as a script in a child process
(`python test_gpu_duplex_ragged.py CASE...`, one line of JSON per case).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":  # the child process: what conftest.py does for pytest
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "noise-c_amd")]

import edge_records as E
from aead_gpu import _filler, check_family, crafted_ragged
from gpu_support import AES, CHACHA, INVALID_PARAM, REC_DT, UNKNOWN_ID, _torch, dev, prepare, stream, sync
from gpu_support import FLAG_CT_GHASH as CT_GHASH, FLAG_FAST as FAST, FLAG_ONE_PASS as ONE_PASS

pytestmark = pytest.mark.gpu

TOO_LONG = 65520
EDGE_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 1400, 16384]
AD_CHOICES = [0, 0, 0, 5, 32]

# What noise_aead_dev_duplex_ragged shares with NOISE_AEAD_RAGGED_DUPLEX unset
# (dispatch.h ragged_duplex_default): the segmented duplex
# beside a one-pass open.  Everything else is reached with the switch at 1,
# in a child process.
def default_on(expect, yflags):
    return expect.startswith("chachapoly_seg_duplex") and bool(yflags & ONE_PASS)


# ------------------------------------------------------------------ the jobs

def oracle_seal(oracle, cipher, keys_flat, key_idx, recs, inp, out, ad):
    """oracle.seal_ragged; a large batch in slices on 16 threads (the C call
    releases the GIL, the records' outputs are disjoint; one call first, so
    that the oracle's S-box exists before the threads start)."""
    n = len(recs)
    if n < 16384:
        return oracle.seal_ragged(cipher, keys_flat, key_idx, recs, inp, out, ad)
    from concurrent.futures import ThreadPoolExecutor
    oracle.encrypt(cipher, bytes(32), 0, b"")
    cuts = [n * t // 16 for t in range(17)]
    with ThreadPoolExecutor(max_workers=16) as pool:
        for f in [pool.submit(oracle.seal_ragged, cipher, keys_flat, key_idx[a:b], recs[a:b], inp, out, ad)
                  for a, b in zip(cuts, cuts[1:])]:
            f.result()


class Job:
    """One ragged job on the host: descriptors, the input image, the output's
    size and prior fill, and what the oracle says of it."""

    def __init__(self, rng, oracle, cipher, lens, state_of, open_, fast, lanes=0, flags=0):
        count = len(lens)
        self.cipher, self.open, self.count, self.lanes = cipher, open_, count, lanes
        self.flags = (FAST if fast else 0) | flags
        self.lens = lens = np.asarray(lens, dtype=np.int64)
        self.refused = lens > 65519
        S = int(state_of.max()) + 1
        self.keys = rng.integers(0, 256, (S, 32), dtype=np.uint8)
        self.state_of = state_of.astype(np.uint32)
        stored = np.minimum(lens, 65519)
        if fast:  # 64-B aligned slots readable to roundup64(max(len, 1)), room for the tag
            slots = (np.maximum(stored, 1) + 16 + 63) // 64 * 64 + 64
        else:     # packed at odd offsets; odd records' input misaligned by 3
            slots = stored + 16 + 5 + 3
        offs = np.zeros(count, dtype=np.int64)
        offs[1:] = np.cumsum(slots)[:-1]
        self.offs = offs
        self.total = total = int(offs[-1] + slots[-1]) + 256
        mis = np.zeros(count, dtype=np.int64) if fast else 3 * (np.arange(count) % 2)
        self.ad = rng.integers(0, 256, count * 64, dtype=np.uint8)
        recs = np.zeros(count, dtype=REC_DT)
        recs["nonce"] = rng.integers(0, 2**62, count, dtype=np.int64).astype(np.uint64)
        recs["ad_off"] = np.arange(count, dtype=np.uint64) * 64
        recs["len"] = lens
        recs["ad_len"] = rng.choice(AD_CHOICES, count)
        self.pt = rng.integers(0, 256, total, dtype=np.uint8)
        keys_flat = np.ascontiguousarray(self.keys.reshape(-1))
        if not open_:
            # out of place: plaintext at in_off of one buffer, CT || tag at out_off of another
            recs["in_off"], recs["out_off"] = offs + mis, offs
            self.inp, self.out_size, self.same_buffer = self.pt, total, False
            self.in_offs, self.out_offs = offs + mis, offs
            self.inplace = np.zeros(count, dtype=bool)
            self.bad = np.zeros(count, dtype=bool)
            self.want_status = np.where(self.refused, 2, 0).astype(np.uint8)
        else:
            # one buffer: CT || tag at [0, total), the out-of-place outputs at
            # [total, 2 total); even records are in place
            self.inplace = ip = np.arange(count) % 2 == 0
            srecs = recs.copy()
            srecs["in_off"] = srecs["out_off"] = offs + mis
            ct = np.full(total, 0x11, dtype=np.uint8)
            oracle_seal(oracle, cipher, keys_flat, self.state_of, srecs, self.pt, ct, self.ad)
            self.bad = bad = (np.arange(count) % 37 == 5) & ~self.refused
            for i in np.nonzero(bad)[0]:
                ct[int(offs[i] + mis[i]) + int(rng.integers(0, int(lens[i]) + 16))] ^= 0x40
            self.given = ct
            self.inp = np.concatenate([ct, np.full(total, 0xA5, dtype=np.uint8)])
            self.in_offs = offs + mis
            self.out_offs = np.where(ip, offs + mis, offs + total)
            recs["in_off"], recs["out_off"] = self.in_offs, self.out_offs
            self.out_size, self.same_buffer = 2 * total, True
            self.want_status = np.where(self.refused, 2, np.where(bad, 1, 0)).astype(np.uint8)
        self.recs = recs

    def on_device(self, aead):
        """Fresh device copies: (NoiseAeadRagged, output tensor, status tensor, keep-alive)."""
        torch = _torch()
        ctx, k = prepare(aead, self.cipher, self.keys)
        recs = self.recs.copy()
        recs["ctx_off"] = self.state_of.astype(np.uint64) * aead.dev_ctx_bytes(self.cipher)
        d_recs, d_in, d_ad = dev(recs.view(np.uint8)), dev(self.inp), dev(self.ad)
        d_out = d_in if self.same_buffer else torch.full((self.out_size,), 0xA5, dtype=torch.uint8, device="cuda")
        d_st = torch.full((self.count,), 9, dtype=torch.uint8, device="cuda")
        job = aead.ragged_job(ctx_base=ctx.data_ptr(), recs=d_recs.data_ptr(), inp=d_in.data_ptr(),
                              out=d_out.data_ptr(), n_records=self.count, status=d_st.data_ptr(),
                              ad=d_ad.data_ptr(), lanes=self.lanes, flags=self.flags)
        return job, d_out, d_st, (ctx, k, d_recs, d_in, d_ad)

    def standalone(self, aead):
        """The job through noise_aead_dev_{seal,open}_ragged on fresh buffers."""
        job, d_out, d_st, keep = self.on_device(aead)
        rc = aead.dev_ragged(self.open, self.cipher, ctx_base=job.ctx_base, recs=job.recs, inp=job.in_,
                             out=job.out, n_records=self.count, status=job.status, ad=job.ad,
                             lanes=self.lanes, flags=self.flags, stream=stream())
        assert rc == 0, hex(rc)
        return d_out, d_st, keep

    def sample(self, rng, full):
        if full:
            return range(self.count)
        pick = set(rng.choice(self.count, min(400, self.count), replace=False).tolist()) | {0, self.count - 1}
        pick |= set(np.nonzero(self.lens > 8192)[0].tolist())
        return sorted(pick)

    def check_oracle(self, oracle, out, st, rng, full, one_pass):
        """out, st: the job's output buffer and statuses after the call."""
        assert np.array_equal(st, self.want_status), np.nonzero(st != self.want_status)[0][:8]
        for i in self.sample(rng, full):
            L, src, dst = int(self.lens[i]), int(self.in_offs[i]), int(self.out_offs[i])
            lab = ("open" if self.open else "seal", i, L)
            if self.refused[i]:  # nothing written
                if self.inplace[i]:
                    assert np.array_equal(out[dst:dst + 64], self.inp[dst:dst + 64]), lab
                else:
                    assert np.all(out[dst:dst + 64] == 0xA5), lab
            elif not self.open:
                a = bytes(self.ad[64 * i:64 * i + int(self.recs["ad_len"][i])])
                exp = oracle.encrypt(self.cipher, bytes(self.keys[self.state_of[i]]), int(self.recs["nonce"][i]),
                                     bytes(self.pt[src:src + L]), a)
                assert bytes(out[dst:dst + L + 16]) == exp, lab
            elif self.bad[i]:
                if self.inplace[i]:
                    assert np.array_equal(out[dst:dst + L + 16], self.given[src:src + L + 16]), lab
                else:  # never written by a verify-first open, zeroed by a one-pass one
                    assert np.all(out[dst:dst + L] == (0 if one_pass else 0xA5)), lab
            else:
                assert np.array_equal(out[dst:dst + L], self.pt[src:src + L]), lab


def duplex_vs_separate(aead, oracle, X, Y, expect, seed, full=True):
    """The three assertions of the module docstring for one call."""
    torch = _torch()
    jx, x_out, x_st, keep_x = X.on_device(aead)
    jy, y_out, y_st, keep_y = Y.on_device(aead)
    rc = aead.dev_duplex_ragged(X.cipher, jx, jy, stream())
    assert rc == 0, hex(rc)
    plan = aead.last_plan()
    sync()
    assert plan.startswith(expect), (plan, expect)                                       # 1
    sx_out, sx_st, keep_sx = X.standalone(aead)
    sy_out, sy_st, keep_sy = Y.standalone(aead)
    sync()
    assert torch.equal(x_out, sx_out), ("seal output", int((x_out != sx_out).sum()))     # 2
    assert torch.equal(y_out, sy_out), ("open output", int((y_out != sy_out).sum()))
    assert torch.equal(x_st, sx_st) and torch.equal(y_st, sy_st), "statuses"
    rng = np.random.default_rng(seed)                                                    # 3
    one_pass = Y.cipher == CHACHA and bool(Y.flags & ONE_PASS) and bool(Y.flags & FAST)
    X.check_oracle(oracle, x_out.cpu().numpy(), x_st.cpu().numpy(), rng, full, False)
    Y.check_oracle(oracle, y_out.cpu().numpy(), y_st.cpu().numpy(), rng, full, one_pass)
    return plan


def small_lens(rng, count):
    lens = rng.integers(0, 3000, count)
    lens[:len(EDGE_LENS)] = EDGE_LENS
    lens[len(EDGE_LENS)] = TOO_LONG
    return lens[rng.permutation(count)]  # descriptors in no particular order


def seg_lens(rng, count):
    """test_gpu_seg.py's _ragged_batch recipe: 0-2600 B, 2 % of 8-60 KiB"""
    lens = rng.integers(0, 2600, count)
    big = rng.choice(count, count // 50, replace=False)
    lens[big] = rng.integers(8192, 61440, len(big))
    lens[0] = TOO_LONG
    return lens[rng.permutation(count)]


def run_states(rng, count, runs):
    """per-state runs of records: windows hold one, two, three and more states"""
    sizes = []
    while sum(sizes) < count:
        sizes.append(int(rng.choice(runs)))
    return np.repeat(np.arange(len(sizes)), sizes)[:count]


def paired_lens(rng, count):
    """test_ragged_aes_paired_windows' recipe"""
    lens = rng.integers(0, 1200, count)
    lens[::211] = 9000
    lens[1] = TOO_LONG
    return lens


# ------------------------------------------------------------------ the cases
# name -> (family or standalone kernel prefix expected, builder(rng, oracle) -> X, Y, full)

def _chacha_windowed(nx, ny, lanes_x, lanes_y, fast, yflags=0):
    def build(rng, oracle):
        X = Job(rng, oracle, CHACHA, small_lens(rng, nx), rng.integers(0, 5, nx), False, fast, lanes_x)
        Y = Job(rng, oracle, CHACHA, small_lens(rng, ny), rng.integers(0, 7, ny), True, fast, lanes_y, yflags)
        return X, Y, True
    return build


def _chacha_seg(nx, ny, yflags=0, lanes_y=0):
    def build(rng, oracle):
        small = ny < 16384
        X = Job(rng, oracle, CHACHA, seg_lens(rng, nx), rng.integers(0, 300, nx), False, True)
        Y = Job(rng, oracle, CHACHA, small_lens(rng, ny) if small else seg_lens(rng, ny),
                rng.integers(0, 300, ny), True, True, lanes_y, yflags)
        return X, Y, False
    return build


def _aes_small(nx, ny, lanes, fast_x, fast_y, flags=0):
    def build(rng, oracle):
        runs = [1, 3, 40, 130, 300]
        X = Job(rng, oracle, AES, small_lens(rng, nx), run_states(rng, nx, runs), False, fast_x, lanes, flags)
        Y = Job(rng, oracle, AES, small_lens(rng, ny), run_states(rng, ny, runs), True, fast_y, lanes, flags)
        return X, Y, True
    return build


def _aes_paired(nx, ny):
    def build(rng, oracle):
        X = Job(rng, oracle, AES, paired_lens(rng, nx), np.arange(nx) // 300, False, True)
        Y = Job(rng, oracle, AES, paired_lens(rng, ny), np.arange(ny) // 300, True, True)
        return X, Y, False
    return build


SHARED = {
    "chacha-k8": ("chachapoly_duplex_ragged<8,true,true>", _chacha_windowed(300, 200, 8, 8, True)),
    "chacha-k4": ("chachapoly_duplex_ragged<4,true,true>", _chacha_windowed(200, 300, 4, 4, True)),
    "chacha-k8-generic": ("chachapoly_duplex_ragged<8,false,false>", _chacha_windowed(300, 200, 8, 8, False)),
    "chacha-k8-one-pass": ("chachapoly_duplex_ragged<8,true,false>", _chacha_windowed(300, 200, 8, 8, True, ONE_PASS)),
    "seg": ("chachapoly_seg_duplex", _chacha_seg(17000, 16400)),
    "seg-one-pass": ("chachapoly_seg_duplex", _chacha_seg(17000, 16400, ONE_PASS)),
    "aes-fast": ("gcm_duplex_ragged<true,256,false,1,4>", _aes_small(700, 450, 4, True, True)),
    "aes-generic": ("gcm_duplex_ragged<false,256,false,1,4>", _aes_small(700, 450, 4, False, False)),
    "aes-fast-ct": ("gcm_duplex_ragged<true,256,true,1,4>", _aes_small(700, 450, 4, True, True, CT_GHASH)),
    "aes-generic-ct": ("gcm_duplex_ragged<false,256,true,1,4>", _aes_small(700, 450, 4, False, False, CT_GHASH)),
    "aes-k8-paired": ("gcm_duplex_ragged<true,1024,false,2,8>", _aes_paired(70000, 66000)),
    "aes-k4-paired": ("gcm_duplex_ragged<true,1024,false,2,4>", _aes_paired(140000, 132000)),
}

NOT_SHARED = {
    "aes-wide": ("gcm_wide<true,", _aes_small(200, 200, 0, True, True)),
    "chacha-lanes-differ": ("chachapoly_open_ragged<8,true,true>", _chacha_windowed(300, 200, 4, 8, True)),
    "aes-fast-on-x-only": ("gcm_ragged_staged<true,false,256,", _aes_small(700, 450, 4, True, False)),
    "chacha-seg-and-windowed": ("chachapoly_open_ragged<", _chacha_seg(17000, 300)),
}
CASES = {**SHARED, **NOT_SHARED}


def family(expect):
    return expect.split("<")[0]


def run_case(aead, oracle, name, expect=None):
    want, build = CASES[name]
    seed = 9000 + sorted(CASES).index(name)
    X, Y, full = build(np.random.default_rng(seed), oracle)
    return duplex_vs_separate(aead, oracle, X, Y, expect or want, seed + 1, full)


# ------------------------------------------------------- the child process

def child(names, switch):
    """Each named case in a fresh process with NOISE_AEAD_RAGGED_DUPLEX=switch;
    {name: (ok, plan or failure text)}."""
    env = dict(os.environ, NOISE_AEAD_RAGGED_DUPLEX=switch)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *names], env=env, capture_output=True,
                       text=True, timeout=600)
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            out[d["case"]] = (d["ok"], d["detail"])
    assert r.returncode == 0 and set(out) == set(names), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return out


_CHILD = {}


def switched_on(name):
    """The result of shared case `name` under NOISE_AEAD_RAGGED_DUPLEX=1: all
    the cases of its family run in one child process, once."""
    group = lambda n: n if "paired" in n else family(SHARED[n][0])  # the large cases: a process each
    if group(name) not in _CHILD:
        _CHILD[group(name)] = child([n for n in SHARED if group(n) == group(name)], "1")
    return _CHILD[group(name)][name]


def main(argv):
    import noise_aead
    import oracle as O
    if not os.path.exists(O.ORACLE_SO):
        O.build(ref=False)
    orc = O.Oracle()
    off = os.environ.get("NOISE_AEAD_RAGGED_DUPLEX") == "0"
    for name in argv:
        try:
            # switch 0: the same results through two standalone launches (the open's is the last)
            expect = ("chachapoly_open_ragged<" if "chacha" in name else "gcm_ragged_staged<true,") if off else None
            detail, ok = run_case(noise_aead, orc, name, expect), True
        except Exception as e:  # an assertion's text goes to the parent
            detail, ok = "%s: %s" % (type(e).__name__, str(e)[:1500]), False
        print(json.dumps({"case": name, "ok": ok, "detail": detail}), flush=True)
    return 0


# ------------------------------------------------------------------ the tests

@pytest.mark.parametrize("name", list(SHARED))
def test_shared_launch_equals_separate_calls(aead, gpu, oracle, name):
    """Two jobs that share a launch: the plan names the shared kernel with the
    jobs' own template arguments, and every byte equals the separate calls'."""
    if default_on(SHARED[name][0], ONE_PASS if "one-pass" in name else 0):
        run_case(aead, oracle, name)
    else:
        ok, detail = switched_on(name)
        assert ok, detail


@pytest.mark.parametrize("name", list(NOT_SHARED))
def test_jobs_that_cannot_share_take_two_launches(aead, gpu, oracle, name):
    """gcm_wide jobs, different lane counts, FAST on one AES-GCM job only, a
    segmented beside a windowed job: the same results, and the last plan is
    the open job's standalone kernel."""
    run_case(aead, oracle, name)


def test_switch_off_takes_two_launches(gpu):
    """NOISE_AEAD_RAGGED_DUPLEX=0 (read once, so a fresh process): shareable
    jobs run as two launches with the same results."""
    for name, (ok, detail) in child(["chacha-k8", "aes-fast"], "0").items():
        assert ok, (name, detail)


def test_default_choice_matches_dispatch(aead, gpu, oracle):
    """With the switch unset a launch is shared exactly where dispatch.h's
    measured default says so (default_on restates it)."""
    if "NOISE_AEAD_RAGGED_DUPLEX" in os.environ:
        return
    for name in ("chacha-k4", "aes-fast", "seg", "seg-one-pass"):
        want, build = SHARED[name]
        X, Y, _ = build(np.random.default_rng(5), oracle)
        jx, _xo, _xs, kx = X.on_device(aead)
        jy, _yo, _ys, ky = Y.on_device(aead)
        assert aead.dev_duplex_ragged(X.cipher, jx, jy, stream()) == 0
        plan = aead.last_plan()
        sync()
        assert plan.startswith(family(want)) == default_on(want, Y.flags), (name, plan)


@pytest.mark.parametrize("cipher", [CHACHA, AES])
def test_empty_job_equals_the_other_jobs_call(aead, gpu, oracle, cipher):
    """n_records == 0 on either side: the call is the other job's standalone call."""
    torch = _torch()
    rng = np.random.default_rng(31 + cipher)
    X = Job(rng, oracle, cipher, small_lens(rng, 120), rng.integers(0, 4, 120), False, True, 4)
    Y = Job(rng, oracle, cipher, small_lens(rng, 90), rng.integers(0, 4, 90), True, True, 4)
    for empty_open in (False, True):
        jx, x_out, x_st, kx = X.on_device(aead)
        jy, y_out, y_st, ky = Y.on_device(aead)
        (jy if empty_open else jx).n_records = 0
        assert aead.dev_duplex_ragged(cipher, jx, jy, stream()) == 0
        live, out, st, idle_out, idle_st = (X, x_out, x_st, y_out, y_st) if empty_open else (Y, y_out, y_st, x_out, x_st)
        s_out, s_st, keep = live.standalone(aead)
        sync()
        assert torch.equal(out, s_out) and torch.equal(st, s_st)
        idle = Y if empty_open else X
        assert torch.equal(idle_out.cpu(), torch.from_numpy(idle.inp) if idle.same_buffer
                           else torch.full((idle.out_size,), 0xA5, dtype=torch.uint8))
        assert bool((idle_st == 9).all())
        live.check_oracle(oracle, out.cpu().numpy(), st.cpu().numpy(), rng, True, False)


def test_arguments(aead, gpu, oracle):
    """A NULL job or NULL descriptors: INVALID_PARAM; status arrays that meet:
    INVALID_PARAM with nothing written; an unknown cipher: UNKNOWN_ID."""
    torch = _torch()
    rng = np.random.default_rng(77)
    X = Job(rng, oracle, CHACHA, small_lens(rng, 100), rng.integers(0, 3, 100), False, True, 8)
    Y = Job(rng, oracle, CHACHA, small_lens(rng, 100), rng.integers(0, 3, 100), True, True, 8)
    jx, x_out, x_st, kx = X.on_device(aead)
    jy, y_out, y_st, ky = Y.on_device(aead)
    assert aead.dev_duplex_ragged(CHACHA, None, jy, stream()) == INVALID_PARAM
    assert aead.dev_duplex_ragged(CHACHA, jx, None, stream()) == INVALID_PARAM
    for job in (jx, jy):
        recs, job.recs = job.recs, None
        assert aead.dev_duplex_ragged(CHACHA, jx, jy, stream()) == INVALID_PARAM
        job.recs = recs
    assert aead.dev_duplex_ragged(0x4303, jx, jy, stream()) == UNKNOWN_ID
    both = torch.full((200,), 9, dtype=torch.uint8, device="cuda")
    jx.status, jy.status = both.data_ptr(), both.data_ptr() + 99  # meet by one byte
    assert aead.dev_duplex_ragged(CHACHA, jx, jy, stream()) == INVALID_PARAM
    sync()
    assert bool((both == 9).all()) and bool((x_st == 9).all()) and bool((y_st == 9).all())
    assert bool((x_out == 0xA5).all()) and torch.equal(y_out.cpu(), torch.from_numpy(Y.inp))
    jy.status = both.data_ptr() + 100                             # touch: independent
    assert aead.dev_duplex_ragged(CHACHA, jx, jy, stream()) == 0
    sync()
    st = both.cpu().numpy()
    assert np.array_equal(st[:100], X.want_status) and np.array_equal(st[100:], Y.want_status)


# ---------------------------------------------------------------- edge values

def edge_check(aead, oracle, cipher, recs, checked, lanes, flags, expect, partner):
    """tests/edge_records.py's crafted records as the open job of a shared
    launch beside an ordinary seal job (and, for check_family's seal step, as
    the seal job beside an ordinary open job): each crafted record opens to its
    plaintext, each of the 128 single-bit tag flips and the first and last
    ciphertext bit is rejected."""
    torch, n = _torch(), len(recs)
    offs, total, (ctx, _k), d_recs, d_ad = crafted_ragged(aead, cipher, recs, True)
    PX, PY = partner

    def run(open_, inplace, buf, init):
        d_in = dev(buf)
        d_out = d_in if inplace else torch.full((total,), init, dtype=torch.uint8, device="cuda")
        d_st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        mine = aead.ragged_job(ctx_base=ctx.data_ptr(), recs=d_recs.data_ptr(), inp=d_in.data_ptr(),
                               out=d_out.data_ptr(), n_records=n, status=d_st.data_ptr(), ad=d_ad.data_ptr(),
                               lanes=lanes, flags=FAST | (flags if open_ else flags & CT_GHASH))
        other, o_out, o_st, keep = (PX if open_ else PY).on_device(aead)
        rc = aead.dev_duplex_ragged(cipher, other if open_ else mine, mine if open_ else other, stream())
        assert rc == 0, hex(rc)
        assert aead.last_plan().startswith(expect), aead.last_plan()
        sync()
        assert np.array_equal(o_st.cpu().numpy(), (PX if open_ else PY).want_status)
        return d_out.cpu().numpy(), d_st.cpu().numpy()

    check_family(recs, run, offs, offs, offs, (total, total, total), (cipher, 0x5A, flags), checked=checked,
                 what=("duplex-ragged", expect, flags))


def edge_case(aead, oracle, name):
    rng = np.random.default_rng(404)
    if name == "chacha":
        recs, checked = E.ragged_shaped(oracle, "chacha").records, None
        partner = [Job(rng, oracle, CHACHA, small_lens(rng, 150), rng.integers(0, 3, 150), o, True, 8)
                   for o in (False, True)]
        for flags in (0, ONE_PASS):
            for p in partner:  # the shared kernel takes the open job's order
                p.flags = FAST | flags
            vf = "false" if flags else "true"
            edge_check(aead, oracle, CHACHA, recs, checked, 8, flags, "chachapoly_duplex_ragged<8,true,%s>" % vf, partner)
    elif name == "seg":
        crafted = E.ragged_shaped(oracle, "seg").records
        recs = _filler(16400, 31)  # pad up to the 16 384-record threshold, as test_ragged_chacha_segmented
        step = len(recs) // len(crafted)
        checked = []
        for k, r in enumerate(crafted):
            checked.append(k * (step + 1) + 7)
            recs.insert(checked[-1], r)
        partner = [Job(rng, oracle, CHACHA, seg_lens(rng, 16500), rng.integers(0, 50, 16500), o, True)
                   for o in (False, True)]
        for flags in (0, ONE_PASS):
            edge_check(aead, oracle, CHACHA, recs, checked, 0, flags, "chachapoly_seg_duplex", partner)
    else:
        recs = E.ragged_shaped(oracle, "aes").records
        partner = [Job(rng, oracle, AES, small_lens(rng, 150), run_states(rng, 150, [1, 3, 40]), o, True, 4)
                   for o in (False, True)]
        for ct in (0, CT_GHASH):
            for p in partner:
                p.flags = FAST | ct
            edge_check(aead, oracle, AES, recs, None, 4, ct,
                       "gcm_duplex_ragged<true,256,%s,1,4>" % ("true" if ct else "false"), partner)
    return "ok"


@pytest.mark.parametrize("name", ["chacha", "seg", "aes"])
def test_edge_values_through_shared_kernels(gpu, name):
    """Poly1305 / GHASH edge values and every tag bit through each of the three
    shared kernels (chachapoly_duplex_ragged, chachapoly_seg_duplex,
    gcm_duplex_ragged), selected by the switch in a child process."""
    ok, detail = child(["edge:" + name], "1")["edge:" + name]
    assert ok, detail


if __name__ == "__main__":
    _run_case = run_case

    def run_case(aead, oracle, name, expect=None):  # "edge:NAME" runs an edge case
        if name.startswith("edge:"):
            return edge_case(aead, oracle, name[5:])
        return _run_case(aead, oracle, name, expect)

    sys.exit(main(sys.argv[1:]))
