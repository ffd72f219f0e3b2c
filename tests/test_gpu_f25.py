"""The X25519 field arithmetic on the device, one operation at a time.

noise_aead_debug_f25_op runs f25_load -> one operation of csrc/fe25519.h ->
f25_store per lane.  Every operation takes every vector of tests/f25_cases.py
in one launch: the edge set E (E x E for add, sub and mul), which
tests/test_dh_host.py proves to take each rare carry path — the second wrap of
f25_fold, the second borrow of f25_sub, freeze's re-carry and its [p, 2^255)
case — and 2000 random operands.  The device build's carry chains are the
__builtin_addc / __builtin_subc forms, which the CPU check of the same header
does not compile, so this is where they meet those paths.

The expectation is Python's integer arithmetic mod p.  freeze must give the
canonical bytes; every other result is compared as int(out) mod p, since any
256-bit representative is a correct raw result.
"""
import functools

import pytest

import f25_cases as F
from gpu_support import dev_bytes

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def expectations(op):
    return tuple(F.expected(op, a, b) for a, b in F.vectors(op))


def launch(aead, torch, op, d_a, d_b, n):
    """One launch of op over n elements into an output with 64 canary bytes on
    each side; (the output tensor, its n values).  Checks the canaries."""
    out = torch.full((64 + 32 * n + 64,), 0xC3, dtype=torch.uint8, device="cuda")
    assert aead.debug_f25_op(F.OPS[op][0], a=d_a, b=d_b, n=n, out=out.data_ptr() + 64,
                             stream=torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:64] == 0xC3).all() and (o[64 + 32 * n:] == 0xC3).all(), "wrote outside d_out[32 n)"
    return out, [int.from_bytes(bytes(r), "little") for r in o[64: 64 + 32 * n].reshape(n, 32)]


def run(aead, torch, op, vecs):
    """op over the (a, b) of vecs; d_b is NULL for a one-operand operation.
    Checks that the operands read back as they were."""
    binary = F.OPS[op][1] == 2
    a = dev_bytes(F.pack([v[0] for v in vecs]))
    b = dev_bytes(F.pack([v[1] for v in vecs])) if binary else None
    before = (a.clone(), b.clone() if binary else None)
    _, got = launch(aead, torch, op, a.data_ptr(), b.data_ptr() if binary else 0, len(vecs))
    assert torch.equal(a, before[0]), "first operands written"
    if binary:
        assert torch.equal(b, before[1]), "second operands written"
    return got


def compare(op, vecs, got, want):
    assert len(got) == len(want) == len(vecs)
    for i, ((a, b), g, w) in enumerate(zip(vecs, got, want)):
        if op == "freeze":
            assert g == w, (op, i, hex(a), hex(g))
        else:
            assert g % F.P == w, (op, i, hex(a), hex(b), hex(g))


@pytest.mark.parametrize("op", F.DEVICE_OPS)
def test_every_vector_in_one_launch(aead, gpu, op):
    import torch
    vecs = F.vectors(op)
    assert len(vecs) % 64 != 0 and len(vecs) > 2000
    compare(op, vecs, run(aead, torch, op, vecs), expectations(op))


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_grid_edge(aead, gpu, n):
    """One lane, a workgroup less one, a whole one, one more: a slice that
    walks through the edges and into the random part."""
    import torch
    for op in F.DEVICE_OPS:
        idx = list(range(7, len(F.vectors(op)), len(F.vectors(op)) // 65))[:n]
        assert len(idx) == n
        vecs = [F.vectors(op)[i] for i in idx]
        compare(op, vecs, run(aead, torch, op, vecs), [expectations(op)[i] for i in idx])


def test_inverse_times_operand_is_one_on_the_device(aead, gpu):
    """invert -> mul with no host round trip: the raw (unreduced) inverse is
    the multiplier's operand as it lies in device memory."""
    import torch
    units = [a for a in F.E if a % F.P]
    assert len(units) == len(F.E) - 3 and {0, F.P, 2 * F.P} <= set(F.E)
    n = len(units)
    d_a = dev_bytes(F.pack(units))
    inv, inv_values = launch(aead, torch, "invert", d_a.data_ptr(), 0, n)
    _, prod = launch(aead, torch, "mul", inv.data_ptr() + 64, d_a.data_ptr(), n)
    for a, i, x in zip(units, inv_values, prod):
        assert i % F.P == pow(a, F.P - 2, F.P), hex(a)
        assert x % F.P == 1, (hex(a), hex(x))
