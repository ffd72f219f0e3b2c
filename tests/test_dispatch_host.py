"""Kernel choice and job checks on the CPU, under ASan/UBSan.

noise-c_amd/csrc/dispatch.h holds, once each, the rules that decide whether a
device job may run and which kernel, grid and arguments it gets.
noise-c_amd/asan/dispatch_check.cpp is a stand-alone program over that header
alone (`make -C noise-c_amd dispatch_check`: g++ -fsanitize=address,undefined
-fno-sanitize-recover=all); it runs here as a plain child process.

Without arguments it runs the job checks: the argument and independence cases
of test_abi.py, pointers, strides and record counts at the arithmetic edges,
and every small job against an enumeration of its records.  With --table it
prints the plan of every case of tests/golden/dispatch_plans.txt.gz — both
ciphers, seal and open, the uniform, duplex and ragged entry points over
record counts, lanes, layouts, records per state, flags, CU counts and every
environment switch — which was recorded from the selection code as it was
before dispatch.h (the launchers' own choices, printed where they launched).
"""
import gzip
import os

from host_check import ROOT, run_check

GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_plans.txt.gz")


def test_job_checks_under_sanitizers():
    line = [l for l in run_check("dispatch_check").stdout.splitlines() if l.startswith("dispatch_check:")][-1].split()
    # the enumeration alone is over a million jobs
    assert int(line[1]) > 1000000 and line[3] == "0", line


def test_plan_table_matches_the_recorded_one():
    want = gzip.open(GOLDEN, "rt").read().splitlines()
    got = run_check("dispatch_check", "--table").stdout.splitlines()
    assert len(want) > 3000
    for n, (g, w) in enumerate(zip(got, want), 1):
        assert g == w, f"line {n}:\n got  {g}\n want {w}"
    assert len(got) == len(want)
