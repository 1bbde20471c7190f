"""Builds one program of tests/cpp against include/rcflow_module.hpp and the product library, for the tests that run it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(name, tmp_path, gxx=False):
    """tests/cpp/<name>.cpp compiled into tmp_path; returns the executable's path.  gxx: with g++ -Wall, as the older
    programs are; otherwise with hipcc -x c++, the flags of tests/cpp's test_module."""
    exe = str(tmp_path / name)
    if gxx:
        front = ["g++", "-O2", "-std=c++17", "-Wall"]
    else:
        front = ["/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc", "-O2", "-std=c++17", "-x", "c++"]
    cmd = front + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                   os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L" + os.path.join(ROOT, "ripcurrents_amd"), "-lrcflow",
                   "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "ripcurrents_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def run(name, tmp_path, *args, gxx=False, timeout=300):
    """builds tests/cpp/<name>.cpp, runs it with `args` and holds it to exit status 0 and its "<name>: ok" line; returns its stdout"""
    r = subprocess.run([build(name, tmp_path, gxx=gxx)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and name + ": ok" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout
