"""The handshake model (tests/handshake_model.py) against the recorded vectors
of tests/golden/vectors: every Curve25519, non-fallback vector of cacophony
and noise-c-basic — every handshake message, every transport message after
the split and, where the file records one, the handshake hash."""
import pytest

import handshake_model as M


@pytest.mark.parametrize("fname,hashes", [("cacophony.txt.gz", 0), ("noise-c-basic.txt.gz", 240)])
def test_model_reproduces_every_25519_vector(oracle, fname, hashes):
    ran = matched = 0
    seen = set()
    for v in M.load_vectors(fname):
        if not M.in_scope(v):
            continue
        matched += M.run_vector(oracle, v)
        ran += 1
        seen.add((v["name"].split("_")[0], v["pattern"]))
    assert ran == 240, "every pattern x cipher x hash x prefix, none skipped"
    assert matched == hashes
    assert seen == {(p, pat) for p in ("Noise", "NoisePSK") for pat in M.PATTERNS}


def test_out_of_scope_vectors_are_the_448_hybrid_and_fallback_ones():
    for fname in ("cacophony.txt.gz", "noise-c-basic.txt.gz", "noise-c-fallback.txt.gz", "noise-c-hybrid.txt.gz"):
        for v in M.load_vectors(fname):
            rc, _ = M.parse_name(v["name"])
            odd = v["dh"] != "25519" or "hybrid" in v or "fallback" in v["name"]
            assert rc == (M.ERROR_NOT_APPLICABLE if odd else 0), v["name"]
