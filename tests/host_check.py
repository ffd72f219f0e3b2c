"""The stand-alone sanitizer programs of noise-c_amd/asan, made and run.

Each `*_check` target is a CPU program over the library's host-only headers,
built with -fsanitize=address,undefined -fno-sanitize-recover=all; the
*_host.py tests run them as plain child processes through run_check."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "noise-c_amd")


def run_check(target, *args, feed=None, timeout=120, checked=True):
    """Make `target` and run noise-c_amd/asan/<target> with args, `feed` on its
    standard input; the finished process.  checked: it exited with status 0
    and neither sanitizer reported anything.  Not checked: a deliberately bad
    case, whose refusal the caller inspects itself."""
    subprocess.run(["make", "-s", "-C", LIB, target], check=True)
    r = subprocess.run([os.path.join(LIB, "asan", target), *args], input=feed, capture_output=True, text=True,
                       timeout=timeout)
    if checked:
        out, tail = r.stdout + r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
        assert r.returncode == 0, "%s exited with %d:\n%s" % (target, r.returncode, tail)
        assert "AddressSanitizer" not in out and "runtime error" not in out, "%s: sanitizer report:\n%s" % (target, tail)
    return r
