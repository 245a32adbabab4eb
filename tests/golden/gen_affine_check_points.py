#!/usr/bin/env python3
"""Generates tests/golden/affine_check_points.npz: G1 points as they arrive IN MEMORY (gnark's
G1Affine: X then Y, six little-endian uint64 words each, Montgomery form with R = 2^384), each with
the status the membership check (curdle_g1_check_batch) owes it WITH and WITHOUT the
prime-order-subgroup test.

Every answer comes from the definitions and the pure-Python oracle (oracle/py/bls12381_ref.py),
never from a kernel of this project, in the order the check decides:
  1. all twelve words zero                      -> INFINITY (gnark's IsInfinity: X and Y both zero)
  2. X or Y, read as a 384-bit integer, >= p    -> BAD_ENCODING (such words are no field element)
  3. not oracle.is_on_curve((x, y))             -> NOT_ON_CURVE   (x, y: the words out of Montgomery form)
  4. oracle.scalar_mul(R, (x, y)) is not None   -> NOT_IN_SUBGROUP (skipped without the subgroup test)
  5.                                            -> OK
No record is skipped anywhere.  Every family also asserts what it was BUILT to be.

Families:
  from_decoder  every record of decode_edge_records.npz that has a point (its g1, torsion -- orders 3,
                11, 10177, 859267, 52437899, with (0, +-2) --, torsion_plus_g1, composite, cleared,
                x_on_curve and sign_edge families), as affine words; the status must be the one that
                file states for the record
  other_curve   points of y^2 = x^3 + b' for b' in 1, 2, 3, 5, 6, 7, 8, 9: eight x each, both signs, with
                (0, +-1) and (0, +-3).  The group law for a = 0 never uses b, so these run through every
                point kernel without a trace, and the subgroup test cannot see b: the curve equation
                is the only thing that stops them, and this family is why the check exists
  mixed         x of one G1 point with y of another; (y, x); (x, y + 1); (x, 0)
  range         a G1 point with X + p, Y + p or both in place of X, Y (they fit in 384 bits and are
                the same residues); a coordinate equal to p; all-ones words; X = 0 with Y >= p
  infinity      (0, 0)

Randomness is SHAKE256 over "<seed>/<tag>", so any entry can be rebuilt without the ones before
it (tests/test_affine_check_fixture.py rebuilds a sample of every family).

Run:  python tests/golden/gen_affine_check_points.py        (a few seconds on one CPU core)
Output: tests/golden/affine_check_points.npz (stored uncompressed with fixed zip timestamps: the
same bytes on every run).
"""
import hashlib
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_decode_edge_records as dec  # noqa: E402  (puts oracle/py on the path)

o = dec.o
SEED = "affine-check-points/1"
OUT = os.path.join(HERE, "affine_check_points.npz")
DECODER_FIXTURE = os.path.join(HERE, "decode_edge_records.npz")
OK, INFINITY, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(5)    # CURDLE_DECODE_* (include/curdle_msm.h)
P, R = o.P, o.R

FAMILIES = ("from_decoder", "other_curve", "mixed", "range", "infinity")
MINIMUM = {"from_decoder": 360, "other_curve": 128, "mixed": 32, "range": 18, "infinity": 1}
OTHER_B = (1, 2, 3, 5, 6, 7, 8, 9)


def draw(tag, mod):
    return int.from_bytes(hashlib.shake_256(f"{SEED}/{tag}".encode()).digest(64), "big") % mod


def g1_point(tag):
    return o.scalar_mul(draw(tag, R - 1) + 1, o.G1)


def mont(v):
    """The 384-bit integer gnark stores for the residue v."""
    return v * o.R_FP % P


def words(X, Y):
    """Twelve uint64 words of the stored integers X, Y (each below 2^384)."""
    assert 0 <= X < 1 << 384 and 0 <= Y < 1 << 384
    return tuple((v >> (64 * i)) & (2 ** 64 - 1) for v in (X, Y) for i in range(6))


def point_words(pt):
    return words(mont(pt[0]), mont(pt[1]))


def expected(w):
    """(status with the subgroup test, status without it) of twelve words, from the definitions."""
    X = sum(int(v) << (64 * i) for i, v in enumerate(w[:6]))
    Y = sum(int(v) << (64 * i) for i, v in enumerate(w[6:]))
    if X == 0 and Y == 0:
        return INFINITY, INFINITY
    if X >= P or Y >= P:
        return BAD_ENCODING, BAD_ENCODING
    pt = (X * o.R_FP_INV % P, Y * o.R_FP_INV % P)
    assert list(o.fp_to_mont_limbs(pt[0])) + list(o.fp_to_mont_limbs(pt[1])) == [int(v) for v in w]
    if not o.is_on_curve(pt):
        return NOT_ON_CURVE, NOT_ON_CURVE
    return (OK if o.scalar_mul(R, pt) is None else NOT_IN_SUBGROUP), OK


# --- the families: generators of (twelve words, built-to-be status with the subgroup test) ---
def fam_from_decoder():
    z = np.load(DECODER_FIXTURE)
    for i in np.nonzero(z["status_no_subgroup"] == OK)[0]:
        b = z["points"][i].tobytes()
        pt = (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))
        assert pt[0] < P and pt[1] < P and o.compress(pt) == z["records"][i].tobytes()
        yield point_words(pt), int(z["status_subgroup"][i])


def other_curve_xs(b):
    """Eight x for which x^3 + b is a non-zero square; x = 0 first where b is a square (b = 1, 9: y = +-1, +-3)."""
    xs = [0] if dec.sqrt_fp(b) is not None and b in (1, 9) else []
    for j in itertools.count():
        if len(xs) == 8:
            return xs
        x = draw(f"other/{b}/{j}", P)
        if dec.sqrt_fp(x * x * x + b) not in (None, 0):
            xs.append(x)


def fam_other_curve():
    for b in OTHER_B:
        for x in other_curve_xs(b):
            y = dec.sqrt_fp(x * x * x + b)
            for q in ((x, y), (x, P - y)):
                assert (q[1] * q[1] - q[0] ** 3 - b) % P == 0 and (q[1] * q[1] - q[0] ** 3 - 4) % P != 0
                yield point_words(q), NOT_ON_CURVE
    assert dec.sqrt_fp(1) in (1, P - 1) and dec.sqrt_fp(9) in (3, P - 3)


def fam_mixed():
    for i in range(8):
        a, b = g1_point(f"mixed/a{i}"), g1_point(f"mixed/b{i}")
        assert a[0] != 0 and a[0] != b[0]
        for q in ((a[0], b[1]), (a[1], a[0]), (a[0], (a[1] + 1) % P), (a[0], 0)):
            assert not o.is_on_curve(q)
            yield point_words(q), NOT_ON_CURVE


def fam_range():
    for i in range(3):
        pt = g1_point(f"range/{i}")
        X, Y = mont(pt[0]), mont(pt[1])
        assert o.scalar_mul(R, pt) is None and X + P < 1 << 384 and Y + P < 1 << 384
        yield words(X + P, Y), BAD_ENCODING                                # the same residues: only the range test sees it
        yield words(X, Y + P), BAD_ENCODING
        yield words(X + P, Y + P), BAD_ENCODING
    pt = g1_point("range/p")
    X, Y = mont(pt[0]), mont(pt[1])
    ones = (1 << 384) - 1
    yield words(P, Y), BAD_ENCODING                                        # a coordinate equal to p
    yield words(X, P), BAD_ENCODING
    yield words(P, P), BAD_ENCODING
    yield words(ones, ones), BAD_ENCODING                                  # all-ones words
    yield words(ones, Y), BAD_ENCODING
    yield words(X, ones), BAD_ENCODING
    yield words(0, P), BAD_ENCODING                                        # X = 0 with Y >= p: not infinity
    yield words(0, Y + P), BAD_ENCODING
    yield words(0, ones), BAD_ENCODING


def fam_infinity():
    yield words(0, 0), INFINITY


GENERATORS = {"from_decoder": fam_from_decoder, "other_curve": fam_other_curve, "mixed": fam_mixed, "range": fam_range,
              "infinity": fam_infinity}


def entries(family, count=None):
    """The first `count` entries of a family (all of them by default) as
    (twelve words, status with the subgroup test, status without it)."""
    out = []
    for w, built in itertools.islice(GENERATORS[family](), count):
        st_sub, st_nosub = expected(w)
        assert built == st_sub, (family, w, built, st_sub)
        assert st_nosub == (OK if st_sub == NOT_IN_SUBGROUP else st_sub)
        out.append((w, st_sub, st_nosub))
    return out


def arrays():
    pts, st_sub, st_nosub, fam = [], [], [], []
    for name in FAMILIES:
        got = entries(name)
        assert len(got) >= MINIMUM[name], (name, len(got))
        print(f"{name:16s} {len(got):4d} points", flush=True)
        for w, a, b in got:
            pts.append(np.array(w, dtype=np.uint64))
            st_sub.append(a)
            st_nosub.append(b)
            fam.append(name)
    return {"points": np.stack(pts), "status_subgroup": np.array(st_sub, dtype=np.uint8),
            "status_no_subgroup": np.array(st_nosub, dtype=np.uint8), "family": np.array(fam, dtype="S16")}


def main():
    o.self_check()
    data = dec.npz_bytes(arrays())
    assert len(data) < 100 * 1024, len(data)
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote", OUT, len(data), "bytes")


if __name__ == "__main__":
    main()
