"""CPU test of the argument rules of the device entry points (ripcurrents_amd/csrc/rc_args.cpp): the unit alone, swept against
the rules stated a second time as interval intersection on integers and modulo tests (tests/cpp/args_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_args_sweep_agrees_with_the_statement_under_asan_and_ubsan():
    """Image form over every size, pixel size, step, base offset and alignment; an array at every position around an image
    in every role; up to three images and two arrays in every role assignment; the in-place pair; null arguments; the
    collector at its capacity.  A child process built with -fsanitize=address,undefined."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "args_check"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "args_check")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.startswith("args_check: ok")
