"""k_scalar_mul_batch_quad (curdle_g1_scalar_mul_batch: out[i] = A[i] + s[i] P[i]) on the scalars at the boundaries
of the GLV split -- one half zero, equal halves, halves with bit 126 set, lambda, -lambda, lambda +- 1, the largest
half (glv_chain_model.special_scalars(); tests/test_glv_chain_model.py shows that their chains meet no exceptional
addition in the model) -- over a random point, G and infinity and over every kind of addend, and at the sizes where
a wave (16 points) or a block (64 points) ends in the middle of the data.  Every output is compared exactly with
A + s P, s P from the C oracle and the sum from the Python oracle."""
import numpy as np
import pytest

import glv_chain_model as M

pytestmark = pytest.mark.gpu

WAVE, BLOCK = 16, 64         # points per wave and per block of k_scalar_mul_batch_quad (four lanes each, 256 lanes a block)
SIZES = [1, 15, 16, 17, 63, 64, 65]
ADDENDS = ("infinity", "-sP", "+sP", "P", "random")


class Ref:
    """s P from the C oracle, computed once per (s, P); points as the Python oracle's affine pairs."""

    def __init__(self, oracle, coracle):
        self.o, self.c, self.cache, self.sums = oracle, coracle, {}, {}

    def mul(self, s, P):
        if P is None or s % M.R == 0:
            return None
        if (s, P) not in self.cache:
            pts = np.array([self.o.affine_to_mont_limbs(P)], dtype=np.uint64)
            sc = np.array([self.o.fr_to_mont_limbs(s)], dtype=np.uint64)
            self.cache[(s, P)] = self.o.jac_from_mont_limbs([int(v) for v in self.c.msm_naive(pts, sc)])
        return self.cache[(s, P)]

    def limbs(self, pts):
        return np.array([self.o.affine_to_mont_limbs(p) for p in pts], dtype=np.uint64).reshape(len(pts), 12)

    def scalars(self, vals):
        return np.array([self.o.fr_to_mont_limbs(v) for v in vals], dtype=np.uint64).reshape(len(vals), 4)

    def check(self, got, P, s, A, what):
        """got[i] == A[i] + s[i] P[i] exactly (A None: no addends)."""
        assert got.shape == (len(P), 12)
        for i in range(len(P)):
            key = (s[i], P[i], A[i] if A is not None else False)
            if key not in self.sums:
                want = self.mul(s[i], P[i])
                self.sums[key] = want if A is None else self.o.add(A[i], want)
            want = self.sums[key]
            assert self.o.affine_from_mont_limbs([int(v) for v in got[i]]) == want, (what, i, hex(s[i]))


@pytest.fixture(scope="module")
def ref(oracle, coracle):
    return Ref(oracle, coracle)


@pytest.fixture(scope="module")
def pool(oracle, coracle):
    """65 points, 65 addends (every seventh infinity) and 65 ordinary scalars: what surrounds the special ones."""
    k, q = oracle.Rand(127).get_frs(2)
    walk = [oracle.affine_from_mont_limbs([int(v) for v in row]) for row in coracle.points_walk(k, q, 2 * SIZES[-1])]
    P, A = walk[:SIZES[-1]], walk[SIZES[-1]:]
    A = [None if i % 7 == 3 else a for i, a in enumerate(A)]
    return P, A, oracle.Rand(128).get_frs(SIZES[-1])


def sweep(oracle, ref, pool, s):
    """The fifteen (P, A) pairs of one scalar: P a random point, G, infinity; A of every kind of ADDENDS."""
    rnd_p, rnd_a = pool[0][5], pool[1][6]
    P, A = [], []
    for pt in (rnd_p, oracle.G1, None):
        sp = ref.mul(s, pt)
        for kind in ADDENDS:
            P.append(pt)
            A.append({"infinity": None, "-sP": oracle.neg(sp), "+sP": sp, "P": pt, "random": rnd_a}[kind])
    return P, A


def test_every_special_scalar_over_every_point_and_addend(gpu, oracle, ref, pool):
    """One scalar per point: every special scalar times (random point, G, infinity) without addends, then with
    an addend of every kind -- infinity, -s P (the result is infinity), +s P (the final addition doubles), P itself,
    a random point."""
    S = M.special_scalars()
    assert len(S) >= 60 and {0, 1, M.LAMBDA, M.R - M.LAMBDA, M.LARGEST_HALF_SCALAR, (1 + M.LAMBDA) << 64} <= set(S)
    P, A, sc = [], [], []
    for s in S:
        p, a = sweep(oracle, ref, pool, s)
        P, A, sc = P + p, A + a, sc + [s] * len(p)
    got = gpu.g1_scalar_mul_batch(ref.limbs(P), ref.scalars(sc), ref.limbs(A))
    ref.check(got, P, sc, A, "addends")
    step = len(ADDENDS)
    got = gpu.g1_scalar_mul_batch(ref.limbs(P[::step]), ref.scalars(sc[::step]))
    ref.check(got, P[::step], sc[::step], None, "no addends")


def test_every_special_scalar_in_the_shared_scalar_form(gpu, oracle, ref, pool):
    """One call per special scalar with that scalar for all points (the fold step's form): the fifteen pairs of
    the sweep and two more, so that the call ends one quad into a second wave."""
    for s in M.special_scalars():
        P, A = sweep(oracle, ref, pool, s)
        P, A = P + P[:2], A + A[3:5]
        assert len(P) == WAVE + 1
        shared = ref.scalars([s])[0]
        ref.check(gpu.g1_scalar_mul_batch(ref.limbs(P), shared, ref.limbs(A)), P, [s] * len(P), A, "shared")
        if s in (0, 1, M.LAMBDA, M.LARGEST_HALF_SCALAR):
            ref.check(gpu.g1_scalar_mul_batch(ref.limbs(P), shared), P, [s] * len(P), None, "shared, no addends")


def special_positions(n):
    """The last quad of a wave and of a block, the first quad of the next, and the last index."""
    want = {WAVE - 1, WAVE, BLOCK - 1, BLOCK, n - 1}
    return sorted(p for p in want if 0 <= p < n)


@pytest.mark.parametrize("n", SIZES)
def test_special_scalars_at_the_edges_of_waves_and_blocks(gpu, oracle, ref, pool, n):
    """n points with ordinary scalars, the special ones taking turns at special_positions(n), where their quad's
    chain differs most from its neighbours' (a zero half skips additions the next quad makes): sizes at which a
    wave or a block is full, one short and one over."""
    P, A, ordinary = pool
    P, A = P[:n], A[:n]
    S = M.special_scalars()
    at = special_positions(n)
    Pl, Al = ref.limbs(P), ref.limbs(A)
    call = 0
    for turn in range(len(at)):                                  # every special scalar comes to every position
        places = at[turn:] + at[:turn]
        for lo in range(0, len(S), len(at)):
            sc = list(ordinary[:n])
            for p, s in zip(places, S[lo:lo + len(at)]):
                sc[p] = s
            if call % 3 == 2:
                ref.check(gpu.g1_scalar_mul_batch(Pl, ref.scalars(sc)), P, sc, None, ("no addends", n, call))
            else:
                ref.check(gpu.g1_scalar_mul_batch(Pl, ref.scalars(sc), Al), P, sc, A, ("addends", n, call))
            call += 1
