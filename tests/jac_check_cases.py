"""The membership check of gnark G1Jac points (curdle_g1_check_jac_batch) as a big-integer rule, and the cases the
tests of its kernel share.  Not a test file: tests/test_jac_check_model.py states what the rule must give,
tests/test_jac_check_gpu.py runs the cases through every build of the kernel.

The rule, per point of 18 words (X, Y, Z in Montgomery form), in this order:
  1. Z all zero words            -> INFINITY (gnark's rule for G1Jac; X and Y are not looked at)
  2. X, Y or Z >= p as integers  -> BAD_ENCODING
  3. Y^2 != X^3 + 4 Z^6          -> NOT_ON_CURVE
  4. with the subgroup test: r (X / Z^2, Y / Z^3) != infinity -> NOT_IN_SUBGROUP   (the definition of G1; oracle/py's law)
  5. OK

The cases derive from the 555 affine points of tests/golden/affine_check_points.npz, whose answers follow from the
definitions alone: each (x, y) becomes (x Z^2, y Z^3, Z) for Z = 1, Z = p - 1 and a seeded random Z.  The curve
equation is homogeneous, so a point of another curve stays off this one and every status carries over; the rows that
are no field elements keep their words and get the Z; the affine infinity (all zero) becomes Z = 0."""
import functools
import hashlib
import os

import numpy as np

import bls12381_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "affine_check_points.npz")
OK, INFINITY, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(5)
TOP = (1 << 384) - 1


def raw(words6):
    """Six uint64 words -> the 384-bit integer they spell (NOT reduced, NOT taken out of Montgomery form)."""
    return sum(int(w) << (64 * i) for i, w in enumerate(words6))


def words_of(X, Y, Z):
    """Three raw 384-bit integers -> 18 words."""
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for v in (X, Y, Z) for i in range(6)]


def mont(v):
    return (v % o.P) * o.R_FP % o.P


@functools.lru_cache(maxsize=None)
def in_g1(pt):
    return o.scalar_mul(o.R, pt) is o.INF


def model_status(words18, subgroup=True):
    X, Y, Z = raw(words18[0:6]), raw(words18[6:12]), raw(words18[12:18])
    if Z == 0:
        return INFINITY
    if X >= o.P or Y >= o.P or Z >= o.P:
        return BAD_ENCODING
    x, y, z = (v * o.R_FP_INV % o.P for v in (X, Y, Z))
    if (y * y - x * x * x - 4 * pow(z, 6, o.P)) % o.P:
        return NOT_ON_CURVE
    if subgroup:
        zi = pow(z, -1, o.P)
        if not in_g1((x * zi * zi % o.P, y * zi * zi * zi % o.P)):
            return NOT_IN_SUBGROUP
    return OK


def seeded(tag):
    """A nonzero field element from a tag."""
    h = b"".join(hashlib.sha256(("jac-check/1/%s/%d" % (tag, j)).encode()).digest() for j in range(2))
    return int.from_bytes(h, "big") % (o.P - 1) + 1


def scaled(x, y, z):
    """Canonical affine (x, y) and z != 0 -> raw Montgomery integers of (x z^2, y z^3, z)."""
    return mont(x * z * z), mont(y * z * z * z), mont(z)


class Cases:
    """points (n, 18) uint64; kind[i] names how case i was made; affine_row[i] is the fixture row a scaled case
    came from (-1: none); want_sub / want_nosub are what the cases were BUILT to be -- the fixture's statuses for the
    scaled ones, the rule's clauses for the rest -- and test_jac_check_model.py holds the model against them."""

    def __init__(self):
        f = np.load(FIXTURE)
        self.fixture = f
        pts, kind, row, sub, nosub = [], [], [], [], []

        def put(w, k, r, s, ns):
            pts.append(w), kind.append(k), row.append(r), sub.append(s), nosub.append(ns)

        g = None
        for i, w in enumerate(f["points"]):
            X, Y = raw(w[:6]), raw(w[6:])
            s, ns = int(f["status_subgroup"][i]), int(f["status_no_subgroup"][i])
            for name, z in (("one", 1), ("minus_one", o.P - 1), ("random", seeded("z/%d" % i))):
                if s == INFINITY:
                    put(words_of(mont(z), mont(z + 1), 0), "scaled_" + name, i, s, ns)      # affine infinity <-> Z = 0
                elif s == BAD_ENCODING:
                    put(words_of(X, Y, mont(z)), "scaled_" + name, i, s, ns)                # no field element: words kept
                else:
                    x, y = X * o.R_FP_INV % o.P, Y * o.R_FP_INV % o.P
                    put(words_of(*scaled(x, y, z)), "scaled_" + name, i, s, ns)
                    if g is None and s == OK:
                        g = (x, y)
        # Z = 0 decides first, whatever X and Y are
        for X, Y in ((0, 0), (mont(g[0]), mont(g[1])), (o.P, o.P + 1), (TOP, TOP), (o.R_FP, o.R_FP), (7, TOP)):
            put(words_of(X, Y, 0), "z_zero", -1, INFINITY, INFINITY)
        # a good point with one coordinate replaced by p, p + 1, 2^384 - 1
        good = scaled(g[0], g[1], seeded("range"))
        for c in range(3):
            for v in (o.P, o.P + 1, TOP):
                t = list(good)
                t[c] = v
                put(words_of(*t), "range_" + "XYZ"[c], -1, BAD_ENCODING, BAD_ENCODING)
        # X scaled by Z, Y by another: off the curve
        for j in range(4):
            z, z2 = seeded("wrong/%d" % j), seeded("wrong2/%d" % j)
            assert pow(z, 3, o.P) != pow(z2, 3, o.P)
            put(words_of(mont(g[0] * z * z), mont(g[1] * z2 * z2 * z2), mont(z)), "wrong_scaling", -1, NOT_ON_CURVE, NOT_ON_CURVE)
        self.points = np.array(pts, dtype=np.uint64)
        self.kind = kind
        self.affine_row = np.array(row)
        self.want_sub = np.array(sub, dtype=np.uint8)
        self.want_nosub = np.array(nosub, dtype=np.uint8)
        self.n = len(pts)
        first = lambda pred: next(i for i in range(self.n) if pred(i))
        fam = [x.decode() for x in f["family"]]
        of = lambda i, name: self.affine_row[i] >= 0 and fam[self.affine_row[i]] == name and kind[i] == "scaled_random"
        # what sits last in a partly filled quad / wave / block (tiled)
        self.first = {"torsion": first(lambda i: of(i, "from_decoder") and self.want_sub[i] == NOT_IN_SUBGROUP),
                      "other_curve": first(lambda i: of(i, "other_curve")),
                      "infinity": first(lambda i: kind[i] == "z_zero"),
                      "g1": first(lambda i: of(i, "from_decoder") and self.want_sub[i] == OK),
                      "range": first(lambda i: kind[i] == "range_Z")}

    def tiled(self, n, last_kind):
        """Indices of n cases, the list repeated and rotated so that case n - 1 is of `last_kind`."""
        return (np.arange(n) + (self.first[last_kind] - (n - 1))) % self.n

    def normalised(self):
        """(rows, affine points): every case with Z != 0 and X, Y, Z < p, taken to affine on the host."""
        rows, aff = [], []
        for i, w in enumerate(self.points):
            X, Y, Z = raw(w[0:6]), raw(w[6:12]), raw(w[12:18])
            if Z == 0 or max(X, Y, Z) >= o.P:
                continue
            x, y, z = (v * o.R_FP_INV % o.P for v in (X, Y, Z))
            zi = pow(z, -1, o.P)
            rows.append(i)
            aff.append(o.fp_to_mont_limbs(x * zi * zi % o.P) + o.fp_to_mont_limbs(y * zi * zi * zi % o.P))
        return np.array(rows), np.array(aff, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def cases():
    return Cases()
