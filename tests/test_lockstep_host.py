"""alg::Lockstep, the rendezvous under curdle_prove_batch, as a stand-alone program (tests/hostbuild/lockstep_flow.cpp)
over the test-only host backend, compiled straight from the compiler with ThreadSanitizer and once more with
AddressSanitizer + UBSan -- no Python and nothing preloaded in the sanitised process.  It runs 1, 2 and 7 members in
lockstep through all five funnels (both routes), a split by whole members, members that throw at the first, a middle and
the last step, a member whose shapes disagree (everyone at that step must get the error), two groups at once, and
curdle_prove_batch against three single calls.  A hang is the failure this guards against: the child gets a timeout."""
import os
import platform
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

HB = os.path.join(ROOT, "tests", "hostbuild")
HOST = os.path.join(ROOT, "go-curdleproofs_amd", "host")
UNITS = ("knobs", "common_rand", "msmaccumulator", "host_ops", "algebra", "transcript", "curdleproofs", "device_accumulator",
         "whisk", "proto_api")
BASE = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", "-O2", "-g"]
IFMA = ["-mavx512f", "-mavx512ifma", "-mavx512vl", "-mavx512bw", "-mavx512dq"]
SANITIZERS = {"thread": ["-fsanitize=thread"],
              "address,undefined": ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


def build(tmp, flags):
    """Every unit on its own compiler process, a few at a time, then the link."""
    cxx = os.environ.get("CXX", "g++")
    cc = lambda *a: subprocess.run([cxx, *BASE, *flags, *a], check=True, capture_output=True, text=True, timeout=900)
    units = [(os.path.join(HOST, u + ".cpp"), []) for u in UNITS]
    units += [(os.path.join(HOST, "host_ops_bmi2.cpp"), ["-mbmi2", "-madx"]), (os.path.join(HOST, "compress_avx512.cpp"), IFMA),
              (os.path.join(HB, "stub_backend.cpp"), []), (os.path.join(HB, "lockstep_flow.cpp"), [])]
    objs = [os.path.join(tmp, os.path.basename(src)[:-4] + ".o") for src, _ in units]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(lambda u: cc("-c", u[0][0], *u[0][1], "-o", u[1]), zip(units, objs)))
    exe = os.path.join(tmp, "lockstep_flow")
    cc(*objs, "-o", exe)
    return exe


@pytest.mark.parametrize("sanitizer", sorted(SANITIZERS))
def test_lockstep_flow_under_the_sanitizer(tmp_path, sanitizer):
    exe = build(str(tmp_path), SANITIZERS[sanitizer])
    cmd = [exe]
    if sanitizer == "thread" and shutil.which("setarch"):
        # GCC's TSan runtime needs its fixed shadow mappings free: no address-space randomisation for the child alone
        cmd = ["setarch", platform.machine(), "-R", exe]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    for report in ("ThreadSanitizer", "ERROR: AddressSanitizer", "runtime error"):
        assert report not in p.stderr, p.stderr
    assert "lockstep_flow OK" in p.stdout
