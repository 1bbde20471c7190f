"""CPU tests of the drop-in boundary and the host logic (no GPU, no compute calls)."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "rcflow.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rcflow_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from ripcurrents_amd import _lib
    lib = _lib.load()                       # raises if the HIP extension is not built
    syms = _declared_symbols()
    assert len(syms) >= 35
    for s in syms:
        assert hasattr(lib, s), "include/rcflow.h declares %s but librcflow.so does not export it" % s
        assert s in _lib.SIGNATURES, "%s has no ctypes signature" % s
    assert set(_lib.SIGNATURES) == set(syms)
    assert lib.rcflow_abi_version() == 1


def test_no_device_fails_loudly_never_falls_back():
    """Without a GPU rcflow_create returns RC_ENODEV and the Python host refuses to run:
    there is no CPU fallback in the product path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ripcurrents_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.rcflow_create(ctypes.byref(h), 0, 640, 480, 1)
    assert rc == -4 and not h.value
    assert b"HIP device" in lib.rcflow_last_error()
    from ripcurrents_amd.api import Context
    with pytest.raises(RuntimeError):
        Context(640, 480)
    assert lib.rcflow_create(ctypes.byref(h), 0, -1, 480, 1) == -1


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under ripcurrents_amd/ may reference it."""
    for base, _, files in os.walk(os.path.join(ROOT, "ripcurrents_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(base, f)).read()
                for pat in ("import oracle", "from oracle", "liboracle", "rc_oracle.h", "oracle/", "oracle."):
                    assert pat not in text, "%s references the oracle (%s)" % (os.path.join(base, f), pat)
    out = subprocess.run(["ldd", os.path.join(ROOT, "ripcurrents_amd", "librcflow.so")], capture_output=True, text=True).stdout
    assert "liboracle" not in out


def test_level_geometry_entry_point_matches_oracle(orc):
    from ripcurrents_amd import _lib
    lib = _lib.load()
    for (w, h, ps, lv) in [(1920, 1080, 0.5, 2), (3840, 2160, 0.5, 4), (640, 480, 0.5, 2), (500, 375, 0.8, 6), (40, 36, 0.5, 3)]:
        for k in range(0, 7):
            wk, hk = ctypes.c_int(), ctypes.c_int()
            L = lib.rcflow_level_geometry(w, h, ps, lv, k, ctypes.byref(wk), ctypes.byref(hk))
            g = orc.level_geometry(w, h, ps, lv, k)
            assert (L, wk.value, hk.value) == (g["levels"], g["w"], g["h"])
    assert lib.rcflow_level_geometry(640, 480, 1.0, 2, 0, None, None) == -1


def test_entry_points_without_a_context_name_themselves_when_they_refuse():
    """Every refusal sets a text that starts with the entry point's name (and names the pointer, where one is null), over the
    text an earlier call left; the codes are the ones these calls always returned."""
    from ripcurrents_amd import _lib
    lib = _lib.load()
    f32, f64, i32 = (ctypes.c_float * 40)(), (ctypes.c_double * 8)(), (ctypes.c_int * 8)()
    names = (ctypes.c_char_p * 2)()
    for name, argtypes in (("rcflow_debug_plan_poly", [ctypes.c_int, ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 6),
                           ("rcflow_debug_plan_poly_folded", [ctypes.c_int, ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 4),
                           ("rcflow_debug_plan_pyr_kernel", [ctypes.c_int, ctypes.c_double, ctypes.c_void_p]),
                           ("rcflow_debug_kind", [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
                           ("rcflow_debug_chain_plan", [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int])):
        getattr(lib, name).argtypes, getattr(lib, name).restype = argtypes, ctypes.c_int
    cases = [("rcflow_level_geometry", (0, 480, 0.5, 2, 0, None, None), None), ("rcflow_level_geometry", (640, 480, 1.0, 2, 0, None, None), None),
             ("rcflow_level_geometry", (640, 480, 0.5, -1, 0, None, None), None), ("rcflow_level_geometry", (640, 480, 0.5, 2, -1, None, None), None),
             ("rcflow_pyrlk_levels", (0, 48, 21, 21, 3), None), ("rcflow_pyrlk_levels", (64, 48, 2, 21, 3), None), ("rcflow_pyrlk_levels", (64, 48, 21, 21, -1), None),
             ("rcflow_jet_lut", (None,), "lut_bgr"),
             ("rcflow_debug_chain_plan", (0, 1080, 32, 8, 0, i32, 8), None), ("rcflow_debug_chain_plan", (1920, 1080, 0, 8, 0, i32, 8), None),
             ("rcflow_debug_chain_plan", (1920, 1080, 32, 8, 0, i32, 1), None), ("rcflow_debug_chain_plan", (1920, 1080, 32, 8, 0, None, 8), "starts"),
             ("rcflow_debug_plan_poly", (0, 1.1, 0, f32, f32, f32, f64, i32, f64), None), ("rcflow_debug_plan_poly", (33, 1.1, 0, f32, f32, f32, f64, i32, f64), None),
             ("rcflow_debug_plan_poly", (5, -1.0, 0, f32, f32, f32, f64, i32, f64), None)]
    cases += [("rcflow_debug_plan_poly", tuple([5, 1.1, 0] + [None if j == i else a for j, a in enumerate((f32, f32, f32, f64, i32, f64))]), nm)
              for i, nm in enumerate(("g", "xg", "xxg", "ig", "n_eff", "kdc"))]
    cases += [("rcflow_debug_plan_poly_folded", (0, 1.1, 0, f32, f32, f32, f64), None)]
    cases += [("rcflow_debug_plan_poly_folded", tuple([5, 1.1, 0] + [None if j == i else a for j, a in enumerate((f32, f32, f32, f64))]), nm)
              for i, nm in enumerate(("qh", "xga", "xgb", "kdch"))]
    cases += [("rcflow_debug_plan_pyr_kernel", (0, 1.0, f32), None), ("rcflow_debug_plan_pyr_kernel", (1024, 1.0, f32), None),
              ("rcflow_debug_plan_pyr_kernel", (5, -1.0, f32), None), ("rcflow_debug_plan_pyr_kernel", (5, 1.0, None), "taps"),
              ("rcflow_debug_kind", (-1, names, names), None), ("rcflow_debug_kind", (25, names, names), None),
              ("rcflow_debug_kind", (0, None, names), "name"), ("rcflow_debug_kind", (0, names, None), "bucket")]
    cases += [("rcflow_profile_enable", (None, 0), "ctx"), ("rcflow_profile_reset", (None,), "ctx"),
              ("rcflow_profile_read", (None, 0, None, None, None, None, None), "ctx"), ("rcflow_profile_read_buckets", (None, None, None), "ctx")]
    for name, args, named in cases:
        assert lib.rcflow_set_option(None, b"chunk", 1) == -1                 # plants the text of another call
        planted = lib.rcflow_last_error()
        assert getattr(lib, name)(*args) == -1, (name, args)
        text = lib.rcflow_last_error().decode()
        assert text != planted.decode() and text.startswith(name + ":"), (name, args, text)
        assert named is None or re.search(r"\b%s\b" % named, text[len(name):]), (name, args, text)
    assert not any(f32) and not any(f64) and not any(i32)                    # nothing was written


def test_level_diagnostics_are_exported_and_refuse_a_null_context():
    """rcflow_debug_level_R / rcflow_debug_level_image read back what the level driver's expansion launches wrote
    (tests/test_gpu_polyexp_forms.py); they are not part of include/rcflow.h and have signatures of their own in _lib.py."""
    from ripcurrents_amd import _lib
    lib = _lib.load()
    assert set(_lib.DEBUG_SIGNATURES) == {"rcflow_debug_level_R", "rcflow_debug_level_image"}
    assert not set(_lib.DEBUG_SIGNATURES) & set(_lib.SIGNATURES)
    out, i32 = (ctypes.c_float * 8)(), ctypes.pointer(ctypes.c_int(7))
    for name in _lib.DEBUG_SIGNATURES:
        assert getattr(lib, name)(None, 0, 0, 0, out, i32, i32) == -1
        assert b"context" in lib.rcflow_last_error()
    assert not any(out) and i32.contents.value == 7


def test_synthetic_clips_are_deterministic():
    from ripcurrents_amd import synth
    a = synth.surf_clip(160, 120, 3, seed=1234)
    b = synth.surf_clip(160, 120, 3, seed=1234)
    assert a.dtype == np.uint8 and a.shape == (3, 120, 160) and np.array_equal(a, b)
    assert not np.array_equal(a, synth.surf_clip(160, 120, 3, seed=1235))
    assert 100 < a.mean() < 156 and 20 < a.std() < 60
    t = synth.translating_clip(64, 48, 2)
    assert t.shape == (2, 48, 64)
    f = synth.rotation_field(640, 480)
    assert f[200, 200, 0] == np.float32(-(200 - 240.0) / 480 * 100)      # main.cpp:376


def test_bench_byte_model_matches_survey():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.survey_model_bytes_per_frame(1920, 1080, 2, 2) == 544838400      # 544.84 MB
    assert bench.survey_model_bytes_per_frame(1920, 1080, 2, 3) == 762566400      # 762.57 MB


def test_segment_bounds_cover_the_clip():
    from ripcurrents_amd.distributed import segment_bounds
    for nframes in (2, 9, 64, 65):
        for world in (1, 2, 3, 8):
            pairs = []
            for r in range(world):
                a, b = segment_bounds(nframes, world, r)
                pairs += [(t, t + 1) for t in range(a, b - 1)]
            assert pairs == [(t, t + 1) for t in range(nframes - 1)]


def test_headers_are_plain_c(tmp_path):
    """The drop-in boundary is a C ABI: include/rcflow.h (and the oracle's header) compile as C99."""
    src = tmp_path / "c99.c"
    src.write_text('#include "rcflow.h"\n#include "rc_oracle.h"\nint main(void) { return RC_OK; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_every_option_is_documented_in_the_header():
    """rcflow_set_option's names (csrc/rcflow_api.hip) all appear in include/rcflow.h's option list."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "ripcurrents_amd", "csrc", "rcflow_api.hip")).read()
    hdr = open(os.path.join(root, "include", "rcflow.h")).read()
    names = set(re.findall(r'strcmp\(name, "([a-z_0-9]+)"\)', src))
    assert len(names) >= 10
    missing = [n for n in sorted(names) if '"%s"' % n not in hdr]
    assert not missing, missing


def test_bench_self_launch_command():
    """`python bench.py --gpus N` without a launcher around it starts one itself (a child process, before any GPU call):
    the same torch.distributed.run line the driver uses, rendezvous on 127.0.0.1, the script's own arguments passed on.
    --dry-launch prints the command instead of running it (no GPU, no torch import)."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "20", "--warmup", "5",
                          "--dry-launch"], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stderr
    cmd = json.loads(out.stdout)["launch"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 1024
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    # one GPU, or a launcher already around the script: nothing to start
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dry-launch"], capture_output=True,
                         text=True, timeout=60, env=env)
    assert json.loads(out.stdout)["launch"] is None
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-launch"], capture_output=True,
                         text=True, timeout=60, env=dict(env, WORLD_SIZE="8", RANK="0", LOCAL_RANK="0"))
    assert json.loads(out.stdout)["launch"] is None


def test_bench_dump_sample_index():
    """bench.py --dump-outputs writes a flow batch beyond its byte share as a sample: one pixel per block of consecutive
    pixels at a seeded offset.  The same indices on every call, ascending without repeats, inside the array, never more
    than asked for, and spread over the whole of it (the headline's 32 fields of 1080p stay under 48 MB)."""
    import numpy as np
    import bench
    n = 32 * 1080 * 1920
    keep = bench.DUMP_FLOW_BYTES // 8
    idx = bench.dump_sample_index(n, keep)
    assert np.array_equal(idx, bench.dump_sample_index(n, keep))
    assert idx.size <= keep and idx.size * 8 > bench.DUMP_FLOW_BYTES // 2 and bench.DUMP_FLOW_BYTES <= 60 << 20
    assert idx[0] >= 0 and idx[-1] < n and (np.diff(idx) > 0).all() and np.diff(idx).max() < 2 * -(-n // keep)
    for n, keep in [(10, 3), (7, 7), (5, 1), (1000, 999)]:
        idx = bench.dump_sample_index(n, keep)
        assert 0 < idx.size <= keep and idx.min() >= 0 and idx.max() < n and (np.diff(idx) > 0).all()


def test_tile_chain_plan_invariants():
    """Host logic of the fused winsize-3 flow kernel's tile chains (option `chain`): the pair groups of a launch cover
    every pair exactly once in order, no group is longer than the option, the groups over the last `chain` pairs halve
    (the launch drains on short blocks), a launch too small to keep ~4 blocks per block slot of the GPU shortens its
    chains or gets none, and chain <= 1 means independent pairs.  Pure host code: runs without a GPU."""
    import ripcurrents_amd
    lib = ripcurrents_amd.load()
    fn = lib.rcflow_debug_chain_plan
    fn.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    fn.restype = ctypes.c_int

    def plan(w, h, pairs, chain, force=0):
        buf = (ctypes.c_int * 80)()
        n = fn(w, h, pairs, chain, force, buf, 80)
        assert n >= 0
        return [buf[i] for i in range(n + 1)] if n else []

    assert plan(1920, 1080, 32, 8) == [0, 8, 16, 24, 28, 30, 31, 32]          # 8, 8, 8, then 4, 2, 1, 1
    assert plan(1920, 1080, 32, 1) == [] and plan(1920, 1080, 1, 8) == []     # independent pairs
    assert plan(480, 270, 32, 8) == []                                        # scale 2 of 1080p: too few blocks for chains
    p1 = plan(960, 540, 32, 8)                                                # scale 1: chains of 4
    assert p1 and max(b - a for a, b in zip(p1, p1[1:])) == 4
    for (w, h, pairs, chain, force) in [(1920, 1080, 32, 8, 0), (3840, 2160, 8, 8, 0), (640, 480, 9, 4, 1), (257, 130, 11, 64, 1),
                                        (1920, 1080, 64, 3, 0), (1920, 1080, 5, 2, 1), (333, 251, 63, 8, 1)]:
        st = plan(w, h, pairs, chain, force)
        assert st, (w, h, pairs, chain)
        lens = [b - a for a, b in zip(st, st[1:])]
        assert st[0] == 0 and st[-1] == pairs and all(l >= 1 for l in lens), st
        assert max(lens) <= chain and len(st) - 1 <= 64
        assert lens[-1] == 1 or pairs <= 1                                    # the launch ends on chains of one
        tail = [l for l in lens if l < max(lens)]
        assert tail == sorted(tail, reverse=True), lens                       # halving tail, never growing again


def test_flow_form_host_logic():
    """rcflow_debug_flow_form: the kernel, tile and grid a flow-iteration launch takes -- rc_flow_form, the function
    rc_launch_flow_iter and rc_launch_flow_iter2 switch on (tests/test_gpu_flow_forms.py asserts it before every case).
    Pure host code: runs without a GPU."""
    from ripcurrents_amd import _lib
    from ripcurrents_amd.api import Context
    form = Context.debug_flow_form
    # the flow diagnostics have a signature table of their own, and the kernel names are RcFlowKernel's, value for value
    assert set(_lib.DEBUG_FLOW_SIGNATURES) == {"rcflow_debug_level_flow", "rcflow_debug_flow_form"}
    assert not set(_lib.DEBUG_FLOW_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.DEBUG_SIGNATURES))
    hdr = open(os.path.join(ROOT, "ripcurrents_amd", "csrc", "rc_common.h")).read()
    enum = re.search(r"enum RcFlowKernel : int \{(.*?)\};", hdr, re.S).group(1)
    assert {int(v): k.lower() for k, v in re.findall(r"RC_FK_(\w+) = (\d+)", enum)} == _lib.FLOW_KERNELS
    out, i32 = (ctypes.c_float * 8)(), ctypes.pointer(ctypes.c_int(7))
    assert _lib.load().rcflow_debug_level_flow(None, 0, 0, 0, 0, out, i32, i32) == -1 and b"context" in _lib.load().rcflow_last_error()
    assert not any(out) and i32.contents.value == 7

    def kt(f):
        return f["kernel"], f["tw"], f["th"]

    # one iteration per launch
    assert kt(form(333, 251, 1, 3)) == ("w3", 64, 16) and kt(form(333, 251, 1, 2, 256)) == ("w3", 64, 16)
    assert kt(form(333, 251, 1, 3, solve=0)) == ("tile", 64, 16) and kt(form(333, 251, 1, 10, 256, solve=0)) == ("tile", 32, 32)
    assert kt(form(333, 251, 1, 5, solve=0)) == ("tile", 64, 16) and kt(form(333, 251, 1, 21, solve=0)) == ("tile", 32, 32)
    assert kt(form(333, 251, 1, 4)) == ("big", 32, 32) and form(333, 251, 1, 5, 256)["nt"] == 512
    assert kt(form(333, 251, 1, 10)) == ("big", 32, 32) and kt(form(333, 251, 1, 11, 256)) == ("big", 32, 32)
    assert kt(form(333, 251, 1, 20, 256)) == ("big", 64, 32) and kt(form(333, 251, 1, 21)) == ("big", 64, 32)
    # the strip sweep: Gaussian m = 5 / 10 from the measured crossovers on, or forced; never for a box window or m = 2
    assert form(333, 217, 1, 20, 256, ablate=8388608)["kernel"] == "sweep" and form(333, 217, 1, 10, 256, ablate=8388608)["kernel"] == "sweep"
    assert form(333, 217, 1, 20, 0, ablate=8388608)["kernel"] == "big" and form(333, 217, 1, 5, 256, ablate=8388608)["kernel"] == "big"
    assert form(1000, 900, 1, 20, 256)["kernel"] == "sweep" and form(1000, 899, 1, 20, 256)["kernel"] == "big"
    assert form(1000, 900, 1, 20, 256, ablate=65536)["kernel"] == "big" and form(1000, 900, 1, 20, 256, ablate=65536 | 8388608)["kernel"] == "big"
    assert form(2000, 1000, 4, 10, 256)["kernel"] == "sweep" and form(2000, 1000, 3, 10, 256)["kernel"] == "big"
    f = form(333, 217, 1, 20, 256, ablate=8388608)
    assert f["tw"] == 64 and f["th"] % 8 == 0 and f["th"] >= 32 and f["tiles_x"] == 6 and f["tiles_y"] == -(-217 // f["th"]) and f["nt"] == 1024
    f = form(1920, 1080, 32, 20, 256)               # 30 strips x 32 pairs: 3 segments of 360 rows
    assert (f["kernel"], f["th"], f["tiles_y"], f["grid_y"]) == ("sweep", 360, 3, 32)
    # any other window: the runtime tile, the best halo efficiency that fits LDS
    def runtime_tile(m):
        best, pick = -1.0, (8, 8)
        for tw, th in ((64, 16), (32, 32), (64, 8), (32, 16), (16, 16), (16, 8), (8, 8)):
            lds = 4 * 5 * ((tw + 2 * m) | 1) * (2 * th + 2 * m)            # M planes of tile + halo, V planes of the tile's rows
            eff = tw * th / ((tw + 2 * m) * (th + 2 * m)) * (0.6 if lds > 64 << 10 else 1.0) * (0.95 if tw < 64 else 1.0)
            if lds <= 150 << 10 and eff > best:
                best, pick = eff, (tw, th)
        return pick

    seen = set()
    for ws in (1, 7, 9, 15, 31, 49):
        for flags in (0, 256):
            f = form(97, 70, 1, ws, flags)
            assert f["kernel"] == "runtime" and (f["tw"], f["th"]) == runtime_tile(ws // 2), (ws, f)
            assert (f["tiles_x"], f["tiles_y"], f["nt"]) == (-(-97 // f["tw"]), -(-70 // f["th"]), 256)
            seen.add((f["tw"], f["th"]))
    assert len(seen) >= 2                            # more than one runtime tile among the windows the GPU test runs
    # two iterations per launch: 28 x 12 below 512 blocks, 28 x 20 below 1024, else 28 x 28; chains always 28 x 28
    for pairs, blocks, nit, d in ((4, 432, 2, 4), (5, 540, 3, 4), (10, 1080, 4, 3)):
        f = form(333, 251, pairs, 3, fuse=2)
        assert 108 * pairs == blocks and (f["kernel"], f["tw"], f["th"], f["nit"], f["d"], f["groups"], f["grid_y"]) == ("rrc", 28, 8 * nit - 4, nit, d, 0, pairs)
        assert f["tiles_x"] == 12 and f["tiles_y"] == -(-251 // f["th"]) and f["nt"] == 256
    f = form(333, 251, 10, 3, fuse=2, chain=8)       # too few blocks for chains unless forced
    assert f["groups"] == 0 and f["nit"] == 4
    f = form(333, 251, 10, 3, fuse=2, chain=8, ablate=33554432)
    assert (f["nit"], f["th"], f["groups"], f["grid_y"]) == (4, 28, 3, 3)            # 10 pairs: chains of 8, 1, 1
    f = form(333, 251, 3, 3, fuse=2, chain=2, ablate=33554432)
    assert (f["nit"], f["groups"]) == (4, 2)                                          # a chained launch is 28 x 28 whatever its size
    assert form(1920, 1080, 32, 3, fuse=2, chain=8)["groups"] == 7
    # interior tiles: the 32 x 8 NIT grid of M, 2 px before the tile, at least 5 px inside the image
    assert form(62, 30, 1, 3, fuse=2)["interior"] == 0 and form(63, 31, 1, 3, fuse=2)["interior"] == 1
    assert form(97, 70, 1, 3, fuse=2)["interior"] == 2 * 4 and form(57, 41, 1, 3, fuse=2)["interior"] == 0
    f = form(333, 251, 10, 3, fuse=2)
    assert f["interior"] == 10 * 7                   # tiles 1..10 of 12, rows 1..7 of 9
    assert form(333, 251, 1, 3)["interior"] == 0     # only the fused kernel has the path
    # refusals: a fused launch of a window that cannot fuse, sizes, a short buffer
    import ctypes as C
    from ripcurrents_amd import _lib
    lib = _lib.load()
    buf = (C.c_int * 16)()
    for args in ((333, 251, 1, 5, 0, 1, 1, 2, 1, 0, 0, buf, 16), (333, 251, 1, 3, 0, 0, 1, 2, 1, 0, 0, buf, 16), (0, 251, 1, 3, 0, 1, 1, 1, 1, 0, 0, buf, 16),
                 (333, 251, 0, 3, 0, 1, 1, 1, 1, 0, 0, buf, 16), (333, 251, 1, 50, 0, 1, 1, 1, 1, 0, 0, buf, 16), (333, 251, 1, 3, 1, 1, 1, 1, 1, 0, 0, buf, 16),
                 (333, 251, 1, 3, 0, 1, 3, 1, 1, 0, 0, buf, 16), (333, 251, 1, 3, 0, 1, 1, 3, 1, 0, 0, buf, 16), (333, 251, 1, 3, 0, 1, 1, 1, 1, 0, 0, buf, 10),
                 (333, 251, 1, 3, 0, 1, 1, 1, 1, 0, 0, None, 16)):
        assert lib.rcflow_debug_flow_form(*args) == -1, args
        assert lib.rcflow_last_error().decode().startswith("rcflow_debug_flow_form:")
    assert not any(buf)


def test_output_validator_refuses_what_is_not_on_the_device():
    import torch
    from ripcurrents_amd.api import _check_out
    dev = torch.device("cuda", 0)
    for t in (None, np.zeros(3), torch.zeros(3, dtype=torch.float64)):      # no tensor at all; a host tensor
        with pytest.raises(ValueError):
            _check_out(t, dev, torch.float64, "out", numel=3)
        with pytest.raises(ValueError):
            _check_out(t, dev, torch.float64, "out", shape=(1, 1, 3), dense=True)
