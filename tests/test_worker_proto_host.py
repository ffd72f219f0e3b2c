"""The resident worker's request protocol on the CPU, under ASan/UBSan.

noise-c_amd/csrc/worker_proto.h holds both halves of the protocol: the
host's encode (stream chunks, header, poison, scrub, stop word) and the rules
the kernel decodes with.  noise-c_amd/asan/worker_proto_check.cpp is a
stand-alone program over that header alone: for both request placements,
seal and open, AD 0..256 and stream totals at every transport edge (len 0,
the head of 3072 / 2048 stream bytes -1 .. +17, the longest record), with
request numbers around every sign and wrap edge, it encodes over exact-size
heap areas, decodes the way aead_worker does and compares byte for byte.
`make -C noise-c_amd worker_proto_check` builds it with
-fsanitize=address,undefined -fno-sanitize-recover=all; it runs here as a
plain child process.
"""
from host_check import run_check


def test_worker_protocol_encode_decode_under_sanitizers():
    r = run_check("worker_proto_check")
    line = [l for l in r.stdout.splitlines() if l.startswith("worker_proto_check:")][-1].split()
    # 2 placements x 2 directions x 6 AD lengths x 8 reachable totals x 4 numbers
    assert int(line[1]) == 768 and line[-2] == "0", r.stdout[-2000:]
