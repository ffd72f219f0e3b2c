"""plan_duplex_ragged and check_duplex_ragged on the CPU, under ASan/UBSan.

`dispatch_check --duplex-ragged` (noise-c_amd/asan/dispatch_check.cpp, the
stand-alone program of test_dispatch_host.py, run as a plain child process)
enumerates both ciphers, 14 record counts and 5 lane counts and 4 flag sets
per job, the NOISE_AEAD_RAGGED_DUPLEX switch on, off and unset, and the
segmented kernel's occupancy known or not, and checks the ragged duplex plan
against plan_ragged — each job's plan alone, the code the ragged entry points
have run since before the duplex existed:

 - a shared plan implies that both standalone plans exist and name one family
   with the same template arguments, and it carries them: sb / ob are the
   standalone grids (window counts for AES-GCM), the grid is sb + ob,
   max(sb, ob) or the persistent bound by family, vf and the open order are
   the open job's;
 - nothing is shared when a job is empty, the switch is off, or family, lanes,
   FAST, shape or CT_GHASH differ;
 - a job plan_ragged refuses is refused with the same rc;
 - check_duplex_ragged at the span edges: status arrays that touch, that meet
   by one byte, at the top of the address space.
"""
from host_check import run_check


def test_duplex_ragged_plans_under_sanitizers():
    line = [l for l in run_check("dispatch_check", "--duplex-ragged").stdout.splitlines() if l.startswith("dispatch_check:")][-1].split()
    assert int(line[1]) > 10000 and line[3].rstrip(",") == "0", line
    assert int(line[5]) > 1000, line  # and the enumeration reached shared plans
