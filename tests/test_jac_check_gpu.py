"""The membership check of gnark G1Jac points (curdle_g1_check_jac_batch, check_kernels.hip) through EVERY build of
its kernel.  The cases and what each must give are tests/jac_check_cases.py's: the 555 points of the affine fixture
scaled by Z = 1, p - 1 and a random Z, Z = 0 over arbitrary X and Y, every coordinate out of range, X and Y scaled
by different Z.  tests/test_jac_check_model.py holds those expectations against the big-integer rule on the CPU.

Builds, forced with the library's own knob (QUAD_MAX_LANES), as for the affine kernel:
  quad   defaults                        k_g1_check_jac<true,true>    (up to 32,768 points)
  lane   QUAD_MAX_LANES=0                k_g1_check_jac<false,true>
  nosub  subgroup_check = False          k_g1_check_jac<false,false>"""
import numpy as np
import pytest

import jac_check_cases as jc

pytestmark = pytest.mark.gpu

BUILD_NAMES = ("quad", "lane", "nosub")
SMALL_SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)          # quad, wave and block tails
LAST_KINDS = ("torsion", "other_curve", "infinity", "g1")     # what sits in the last, partly filled quad / block


@pytest.fixture(scope="module")
def cs():
    return jc.cases()


def run_build(gpu, build, pts, device=False, stream=None):
    import torch
    sub = build != "nosub"
    if device:
        d = torch.from_numpy(np.ascontiguousarray(pts).view(np.int64)).to("cuda:0")
        call = lambda: gpu.g1_check_jac_batch_device(d.data_ptr(), len(pts), sub, stream=stream)
    else:
        call = lambda: gpu.g1_check_jac_batch(pts, sub)
    if build == "lane":
        with gpu.knobs(QUAD_MAX_LANES=0):
            return call()
    return call()


def check_build(gpu, cs, build, idx, device=False):
    want = cs.want_nosub[idx] if build == "nosub" else cs.want_sub[idx]
    got = run_build(gpu, build, cs.points[idx], device)
    bad = np.nonzero(got != want)[0]
    print("build %s%s n=%d: %d of %d statuses differ" % (build, " (device)" if device else "", len(idx), len(bad), len(idx)))
    assert got.shape == want.shape and len(bad) == 0, \
        (build, len(idx), [(int(i), cs.kind[idx[i]], "want %d got %d" % (want[i], got[i])) for i in bad[:12]], len(bad))


def test_cases_are_whole(cs):
    assert cs.n >= 3 * 555 + 6 + 9 + 4
    assert set(cs.want_sub.tolist()) == {0, 1, 2, 3, 4} and set(cs.want_nosub.tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("build", BUILD_NAMES)
def test_every_case_through_every_build(gpu, cs, build):
    check_build(gpu, cs, build, np.arange(cs.n))


@pytest.mark.parametrize("build", BUILD_NAMES)
def test_every_case_from_a_resident_array(gpu, cs, build):
    check_build(gpu, cs, build, np.arange(cs.n), device=True)


def test_a_resident_array_on_the_callers_stream(gpu, cs):
    import torch
    s = torch.cuda.Stream()
    got = run_build(gpu, "quad", cs.points, device=True, stream=s.cuda_stream)
    assert (got == cs.want_sub).all()


@pytest.mark.parametrize("n", SMALL_SIZES)
def test_tails_of_quads_waves_and_blocks(gpu, cs, n):
    """Batch sizes that leave the last quad of lanes, wave and block partly empty; which kind of point comes last
    rotates with the size and the build, so that every kind is last in every build."""
    for r, build in enumerate(BUILD_NAMES):
        kind = LAST_KINDS[(SMALL_SIZES.index(n) + r) % len(LAST_KINDS)]
        idx = cs.tiled(n, kind)
        assert idx[-1] == cs.first[kind]
        check_build(gpu, cs, build, idx)


def test_rotation_puts_every_kind_last_in_every_build():
    for r in range(len(BUILD_NAMES)):
        assert {LAST_KINDS[(i + r) % len(LAST_KINDS)] for i in range(len(SMALL_SIZES))} == set(LAST_KINDS)


@pytest.mark.parametrize("n", [32768, 32769])
def test_the_boundary_where_the_build_changes(gpu, cs, n):
    """32,768 points are the last launch on four lanes per point, 32,769 the first on one lane."""
    check_build(gpu, cs, "quad", cs.tiled(n, "torsion" if n == 32768 else "other_curve"))


def test_agreement_with_the_affine_check(gpu, cs):
    """Every case with Z != 0 and X, Y, Z < p, taken to affine on the host: the affine kernel says of the normalised
    point what the Jacobian kernel says of the point as it lies, with and without the subgroup test."""
    rows, aff = cs.normalised()
    assert len(rows) >= 3 * 500
    for sub in (True, False):
        a = gpu.g1_check_batch(aff, sub)
        j = gpu.g1_check_jac_batch(cs.points[rows], sub)
        assert (a == j).all(), [(int(rows[i]), cs.kind[rows[i]], int(a[i]), int(j[i])) for i in np.nonzero(a != j)[0][:12]]
    assert {int(s) for s in j} == {0, 3}
