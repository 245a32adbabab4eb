"""The batched point decoder's subgroup test on the records an attacker would send, through EVERY
build of the device code that decides it.

tests/golden/decode_edge_records.npz (generator beside it) holds 460 records whose answers follow
from the definitions alone -- [r] P == inf with the textbook oracle, Euler's criterion, the encoding
rules: points of order 3, 11, 10177, 859267 and 52437899 (the prime factors of the cofactor; order 3
is (0, +-2), where beta x = 0 and phi(P) = P), sums T + Q of those with G1 points, composite orders,
cofactor-cleared points, x and sign-threshold edges, malformed encodings.  No record is skipped.

Routes, forced with the library's own knobs (TWO_KERNEL_MAX, QUAD_MAX_LANES):

  A  defaults, one-shot                  k_g1_decompress<false,false> + k_g1_subgroup_from_x<true>
  B  TWO_KERNEL_MAX=0                    k_g1_decompress<true,true>: the fused quad kernel, which a
                                         one-shot decoding takes when every decode context is busy
  C  TWO_KERNEL_MAX=0, QUAD_MAX_LANES=0  k_g1_decompress<false,true>
  D  QUAD_MAX_LANES=0, begin / finish    k_g1_decompress<false,false> + k_g1_subgroup_from_x<false>
  E  one-shot without the subgroup test  k_g1_decompress<false,false> alone
  F  start / points / finish             as A

test_kernel_trace_names_all_five_builds proves with a kernel trace that A-D run the kernels named."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "decode_edge_records.npz")
ROUTES = "ABCDEF"
SMALL_SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)          # quad, wave and block tails
LAST_KINDS = ("torsion", "off_curve", "infinity", "g1")       # what sits in the last, partly filled quad / block


class Edge:
    def __init__(self, oracle):
        z = np.load(FIXTURE)
        self.recs = z["records"]
        self.st_sub = z["status_subgroup"]
        self.st_nosub = z["status_no_subgroup"]
        self.family = [f.decode() for f in z["family"]]
        self.n = len(self.recs)
        # the oracle's affine point in gnark's Montgomery layout, zeros where the record has no point
        self.words = np.zeros((self.n, 12), dtype=np.uint64)
        for i, row in enumerate(z["points"]):
            if self.st_nosub[i] == 0:
                b = row.tobytes()
                x, y = int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big")
                assert x < oracle.P and y < oracle.P
                self.words[i] = oracle.fp_to_mont_limbs(x) + oracle.fp_to_mont_limbs(y)
        first = lambda pred: next(i for i in range(self.n) if pred(i))
        self.first = {"torsion": first(lambda i: self.family[i] == "torsion"),
                      "off_curve": first(lambda i: self.family[i] == "x_off_curve"),
                      "infinity": first(lambda i: self.st_sub[i] == 1),
                      "g1": first(lambda i: self.family[i] == "g1")}

    def tiled(self, n, last_kind):
        """Indices of n records, the fixture repeated and rotated so that record n - 1 is of `last_kind`."""
        return (np.arange(n) + (self.first[last_kind] - (n - 1))) % self.n


def attack_records(oracle):
    """Three records of the fixture for the consumers' case pools (tracker batch, Whisk batch, protocol): the point
    (0, 2) of order 3, a point of order 11, and T + Q with T of order 10177 and Q in G1 -- each checked here against
    the definition again, so that a consumer's test says what it planted."""
    z = np.load(FIXTURE)
    fam = z["family"]
    point = lambda i: (int.from_bytes(z["points"][i, :48].tobytes(), "big"), int.from_bytes(z["points"][i, 48:].tobytes(), "big"))
    tors = np.nonzero(fam == b"torsion")[0]
    tq = np.nonzero(fam == b"torsion_plus_g1")[0]
    i3, i11, itq = int(tors[0]), int(tors[16]), int(tq[32])
    assert point(i3) == (0, 2) and oracle.scalar_mul(3, point(i3)) is None
    assert point(i11) is not None and oracle.scalar_mul(11, point(i11)) is None
    assert oracle.scalar_mul(oracle.R, point(itq)) is not None and oracle.scalar_mul(10177 * oracle.R, point(itq)) is None
    out = {"order 3": z["records"][i3].tobytes(), "order 11": z["records"][i11].tobytes(), "T+Q": z["records"][itq].tobytes()}
    assert all(z["status_subgroup"][i] == 4 and oracle.compress(point(i)) == rec
               for i, rec in zip((i3, i11, itq), out.values()))
    return out


@pytest.fixture(scope="module")
def edge(oracle):
    return Edge(oracle)


def run_route(gpu, route, blob, n):
    """-> (points, final status, preliminary status or None)"""
    if route == "A":
        pts, st = gpu.g1_decompress_batch(blob, True)
        return pts, st, None
    if route == "B":
        with gpu.knobs(TWO_KERNEL_MAX=0):
            pts, st = gpu.g1_decompress_batch(blob, True)
        return pts, st, None
    if route == "C":
        with gpu.knobs(TWO_KERNEL_MAX=0, QUAD_MAX_LANES=0):
            pts, st = gpu.g1_decompress_batch(blob, True)
        return pts, st, None
    if route == "D":
        with gpu.knobs(QUAD_MAX_LANES=0):
            pts, pre, ticket = gpu.g1_decompress_begin(blob)
            return pts, gpu.g1_decompress_finish(ticket, n), pre
    if route == "E":
        pts, st = gpu.g1_decompress_batch(blob, False)
        return pts, st, None
    if route == "F":
        ticket = gpu.g1_decompress_start(blob)
        try:
            pts, pre = gpu.g1_decompress_points(ticket, n)
        except Exception:
            gpu.g1_decompress_finish(ticket, n)
            raise
        return pts, gpu.g1_decompress_finish(ticket, n), pre
    raise AssertionError(route)


def mismatches(edge, idx, got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return [(int(i), edge.family[idx[i]], "want %d got %d" % (want[i], got[i])) for i in bad[:12]], len(bad)


def check_route(gpu, edge, route, idx):
    """One run of `route` over the fixture records idx[0..n): every status and every output word."""
    n = len(idx)
    blob = edge.recs[idx].tobytes()
    pts, st, pre = run_route(gpu, route, blob, n)
    assert pts.shape == (n, 12) and st.shape == (n,)
    want_final = edge.st_nosub[idx] if route == "E" else edge.st_sub[idx]
    print("route %s n=%d: %d of %d statuses differ from the fixture" % (route, n, int((st != want_final).sum()), n))
    assert (st == want_final).all(), (route, n) + mismatches(edge, idx, st, want_final)
    if route in "ABC":
        # the one-shot entry point promises zeros for every record that is not a usable point
        want_pts = np.where((edge.st_sub[idx] == 0)[:, None], edge.words[idx], 0)
    else:
        # E has no subgroup verdict; the two- and three-step forms hand the point back BEFORE the verdict:
        # a curve point outside G1 arrives as itself, and only the final status says what it is
        want_pts = edge.words[idx]
    if pre is not None:
        assert (pre == edge.st_nosub[idx]).all(), (route, n) + mismatches(edge, idx, pre, edge.st_nosub[idx])
    rows = np.nonzero((pts != want_pts).any(axis=1))[0]
    assert len(rows) == 0, (route, n, [(int(i), edge.family[idx[i]], int(want_final[i])) for i in rows[:12]], len(rows))
    return pts, st


def test_fixture_is_whole(edge):
    from collections import Counter
    count = Counter(edge.family)
    minimum = {"g1": 138, "torsion": 80, "torsion_plus_g1": 80, "composite": 24, "cleared": 16, "x_on_curve": 14,
               "x_off_curve": 69, "sign_edge": 8, "encoding": 10}
    assert all(count[f] >= m for f, m in minimum.items()), count
    assert set(edge.st_sub.tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_record_through_every_build(gpu, edge, route):
    check_route(gpu, edge, route, np.arange(edge.n))


def test_routes_agree_byte_for_byte(gpu, edge):
    idx = np.arange(edge.n)
    blob = edge.recs.tobytes()
    out = {r: run_route(gpu, r, blob, edge.n) for r in "ABCD"}
    for r in "BCD":
        assert out[r][1].tobytes() == out["A"][1].tobytes(), (r,) + mismatches(edge, idx, out[r][1], out["A"][1])
    for r in "BC":
        assert out[r][0].tobytes() == out["A"][0].tobytes(), r
    # D returned its points before the verdict; with the rejected ones blanked as the one-shot form does, the same bytes
    d_pts = np.where((out["D"][1] == gpu.DECODE_NOT_IN_SUBGROUP)[:, None], 0, out["D"][0]).astype(np.uint64)
    assert d_pts.tobytes() == out["A"][0].tobytes()


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_tails_of_quads_waves_and_blocks(gpu, edge, n):
    """Batch sizes that leave the last quad-of-lanes group, wave and block partly empty; which kind of
    record comes last rotates with the size and the route, so that every kind is last in every route."""
    for r, route in enumerate("ABCD"):
        kind = LAST_KINDS[(SMALL_SIZES.index(n) + r) % len(LAST_KINDS)]
        idx = edge.tiled(n, kind)
        assert idx[-1] == edge.first[kind]
        check_route(gpu, edge, route, idx)


def test_rotation_puts_every_kind_last_in_every_route():
    for r in range(4):
        assert {LAST_KINDS[(i + r) % len(LAST_KINDS)] for i in range(len(SMALL_SIZES))} == set(LAST_KINDS)


@pytest.mark.parametrize("n", [32768, 32769])
def test_the_boundary_where_the_build_changes(gpu, edge, n):
    """32,768 records are the last batch on four lanes per point, 32,769 the first on one lane, for the one-shot
    form (two kernels, then the fused one-lane kernel) and for the subgroup kernel of the two-step form; the fused
    quad kernel gets its largest launch too."""
    for route, kind in (("A", "torsion"), ("F", "off_curve"), ("E", "infinity")) + ((("B", "torsion"),) if n == 32768 else ()):
        check_route(gpu, edge, route, edge.tiled(n, kind))


CHILD = r"""
import sys
sys.path[:0] = [%(pkg)r, %(tests)r]
import numpy as np
import curdlemsm as cm
cm.init(0)
z = np.load(%(fixture)r)
blob, want, n = z["records"].tobytes(), z["status_subgroup"], len(z["records"])
got = [cm.g1_decompress_batch(blob, True)[1]]
with cm.knobs(TWO_KERNEL_MAX=0):
    got.append(cm.g1_decompress_batch(blob, True)[1])
with cm.knobs(TWO_KERNEL_MAX=0, QUAD_MAX_LANES=0):
    got.append(cm.g1_decompress_batch(blob, True)[1])
with cm.knobs(QUAD_MAX_LANES=0):
    _, _, t = cm.g1_decompress_begin(blob)
    got.append(cm.g1_decompress_finish(t, n))
assert all((g == want).all() for g in got), [int((g != want).sum()) for g in got]
print("routes A-D ran")
"""

BUILDS = {"k_g1_decompress<true,true>": r"k_g1_decompress<true,\s*true>|k_g1_decompressILb1ELb1EE",
          "k_g1_decompress<false,true>": r"k_g1_decompress<false,\s*true>|k_g1_decompressILb0ELb1EE",
          "k_g1_decompress<false,false>": r"k_g1_decompress<false,\s*false>|k_g1_decompressILb0ELb0EE",
          "k_g1_subgroup_from_x<true>": r"k_g1_subgroup_from_x<true>|k_g1_subgroup_from_xILb1EE",
          "k_g1_subgroup_from_x<false>": r"k_g1_subgroup_from_x<false>|k_g1_subgroup_from_xILb0EE"}


@pytest.mark.timeout(400)
def test_kernel_trace_names_all_five_builds(gpu):
    """A child process under the profiler's kernel trace runs routes A-D once on the fixture; its statistics must
    name every build of both kernels -- the proof that route B is the fused quad kernel and not a second run of A."""
    prof = shutil.which("rocprofv3") or (os.path.exists("/opt/rocm/bin/rocprofv3") and "/opt/rocm/bin/rocprofv3")
    if not prof:
        pytest.fail("rocprofv3 is not on this machine's path: the kernel trace cannot be taken")
    code = CHILD % {"pkg": os.path.join(ROOT, "go-curdleproofs_amd"), "tests": os.path.join(ROOT, "tests"), "fixture": FIXTURE}
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["timeout", "-k", "10", "300", prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d,
                            "-o", "decode", "--", sys.executable, "-c", code], capture_output=True, text=True, timeout=360)
        assert p.returncode == 0 and "routes A-D ran" in p.stdout, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
        text = ""
        for path in glob.glob(os.path.join(d, "**", "*.csv"), recursive=True):
            with open(path, errors="replace") as f:
                text += f.read()
    assert text, "the profiler wrote no csv"
    named = {b: bool(re.search(pat, text)) for b, pat in BUILDS.items()}
    print(named)
    assert all(named.values()), named
