"""The CRS import and export as a stand-alone program (tests/hostbuild/crs_import_flow.cpp) over the test-only host
backend, compiled straight from the compiler with AddressSanitizer + UBSan -- no Python and nothing preloaded in the
sanitised process.  The program checks that a TRUSTED import of an exported CRS proves the generated handle's bytes from
the same seeds at ell = 4 and 12 and that either handle verifies them, every refusal and every fault (*out NULL, the
fault record, the text; the leak check is the witness that each way out frees what it allocated), the order point fault,
duplicate, sum, and import, free, import again.  The child gets a timeout."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from conftest import ROOT

HB = os.path.join(ROOT, "tests", "hostbuild")
HOST = os.path.join(ROOT, "go-curdleproofs_amd", "host")
UNITS = ("knobs", "common_rand", "msmaccumulator", "host_ops", "algebra", "transcript", "curdleproofs", "device_accumulator",
         "whisk", "proto_api")
BASE = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-O2", "-g"]
IFMA = ["-mavx512f", "-mavx512ifma", "-mavx512vl", "-mavx512bw", "-mavx512dq"]
SANITIZE = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build(tmp):
    """Every unit on its own compiler process, a few at a time, then the link."""
    cxx = os.environ.get("CXX", "g++")
    cc = lambda *a: subprocess.run([cxx, *BASE, *SANITIZE, *a], check=True, capture_output=True, text=True, timeout=900)
    units = [(os.path.join(HOST, u + ".cpp"), []) for u in UNITS]
    units += [(os.path.join(HOST, "host_ops_bmi2.cpp"), ["-mbmi2", "-madx"]), (os.path.join(HOST, "compress_avx512.cpp"), IFMA),
              (os.path.join(HB, "stub_backend.cpp"), []), (os.path.join(HB, "crs_import_flow.cpp"), [])]
    objs = [os.path.join(tmp, os.path.basename(src)[:-4] + ".o") for src, _ in units]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda u: cc("-c", u[0][0], *u[0][1], "-o", u[1]), zip(units, objs)))
    exe = os.path.join(tmp, "crs_import_flow")
    cc(*objs, "-o", exe)
    return exe


def test_crs_import_flow_under_the_sanitizer(tmp_path):
    exe = build(str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    for report in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error"):
        assert report not in p.stderr, p.stderr
    assert "crs_import_flow OK" in p.stdout
