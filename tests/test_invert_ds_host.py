"""csrc/invert_ds.h as a stand-alone program (tests/hostbuild/invert_ds_flow.cpp), compiled straight from the compiler
with AddressSanitizer + UBSan -- no Python and nothing preloaded in the sanitised process.  The test writes the cases of
the big-integer model (tests/fp_divsteps_model.py) to a file under tmp_path; the program runs the header's body, its
repackings and both entry forms on them and prints the words, which are compared with the model bit for bit.  A signed
shift or a signed overflow in the limb code ends the program (-fno-sanitize-recover).  Word patterns at or above p run
too: nothing is compared there, the sanitizers are the check.  The child gets a timeout."""
import os
import subprocess

import fp_divsteps_model as m
from conftest import ROOT

HB = os.path.join(ROOT, "tests", "hostbuild")
BASE = ["-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-O1", "-g"]
SANITIZE = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_invert_ds_flow_under_the_sanitizer(tmp_path):
    exe = str(tmp_path / "invert_ds_flow")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, *BASE, *SANITIZE, os.path.join(HB, "invert_ds_flow.cpp"), "-o", exe], check=True,
                   capture_output=True, text=True, timeout=600)
    gnark = m.all_cases()
    raw = m.all_cases()[:300] + list(m.RAW_EXTRA) + [c + m.P for c in m.fixed_cases()[:9] if c + m.P < 2 * m.P]
    over = [m.P, m.P + 1, (1 << 384) - 1, (1 << 383) + 12345]
    cases = tmp_path / "cases.txt"
    cases.write_text("".join(f"G {a:x}\n" for a in gnark) + "".join(f"R {a:x}\n" for a in raw) + "".join(f"X {a:x}\n" for a in over))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, str(cases)], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    for report in ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error"):
        assert report not in p.stderr, p.stderr
    lines = p.stdout.split("\n")
    assert lines[len(gnark) + len(raw) + len(over)] == f"invert_ds_flow OK {len(gnark) + len(raw) + len(over)}"
    for a, line in zip(gnark, lines):
        y, viol = m.invert_gnark(a)
        assert y == m.want_gnark(a)
        assert line == "G %x " % viol + " ".join("%x" % w for w in m.limbs(y, 32, 12)), hex(a)
    for a, line in zip(raw, lines[len(gnark):]):
        y, viol = m.invert_raw28(a)
        assert line == "R %x " % viol + " ".join("%x" % w for w in m.limbs28(y)), hex(a)
    for line in lines[len(gnark) + len(raw):len(gnark) + len(raw) + len(over)]:
        assert line in ("X 0", "X 1")
