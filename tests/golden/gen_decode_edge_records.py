#!/usr/bin/env python3
"""Generates tests/golden/decode_edge_records.npz: 48-byte compressed-G1 records at the edges
of the batched point decoder, each with the status the decoder owes it WITH and WITHOUT the
prime-order-subgroup test and the affine point it owes for a usable record.

Everything comes from the pure-Python oracle (oracle/py/bls12381_ref.py) and the definitions,
never from a decoder of this project:
  * encoding rules: bit 7 of byte 0 = compressed (must be set on this wire), bit 6 = infinity
    (then every other bit must be clear), bit 5 = "y is the larger root" (y > (p - 1) / 2);
    the remaining 381 bits are x, big-endian, and must be < p;
  * on the curve: x^3 + 4 is a square (Euler's criterion), y by pow(., (p + 1) / 4);
  * in the subgroup: oracle.scalar_mul(R, pt) is None, i.e. [r] P == inf.
Every family also asserts what it was BUILT to be (order of T exactly l, [r](T + Q) != inf,
[r](h Q) == inf, Euler's criterion for the off-curve x, ...), so an answer in the file has two
independent reasons.

The cofactor of G1 in E(Fp) is h = (z - 1)^2 / 3 = 3 * 11^2 * 10177^2 * 859267^2 * 52437899^2;
the l-part of the group is Z_l x Z_l (order 3: Z_3), so (h r / l^2) Q has order l or 1.

Sign edges.  p = 1 mod 9 (p - 1 = 3^2 * t), so cube roots need more than one power: the
roots are found by taking a^(1/3 mod t) and correcting it inside the 9-element 3-Sylow subgroup
by search (cube_roots below).  y = (p - 1) / 2 - 4 is the value nearest below the sign threshold
for which y^2 - 4 is a cube; its negative is (p - 1) / 2 + 5, the nearest above, so the two are
the SAME curve points seen through the two sign flags.  The family therefore holds the three
points (x, beta x, beta^2 x) of each of the four nearest such y (d = 4, 7, 8, 14), each
with each flag: 24 records whose comparison with (p - 1) / 2 is decided in the lowest limb alone.

Randomness is SHAKE256 over "<seed>/<family>/<index>", so any entry can be rebuilt without the
ones before it (tests/test_decode_edge_fixture.py rebuilds a sample of every family).

Run:  python tests/golden/gen_decode_edge_records.py       (7 s on one CPU core)
Output: tests/golden/decode_edge_records.npz (stored uncompressed with fixed zip timestamps:
the same bytes on every run).
"""
import functools
import hashlib
import io
import itertools
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle", "py"))
import bls12381_ref as o  # noqa: E402

SEED = "decode-edge-records/1"
OUT = os.path.join(HERE, "decode_edge_records.npz")
OK, INFINITY, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(5)    # CURDLE_DECODE_* (include/curdle_msm.h)

P, R = o.P, o.R
HALF = (P - 1) // 2
Z = -0xD201000000010000
H = (Z - 1) ** 2 // 3
PRIMES = (3, 11, 10177, 859267, 52437899)
assert H == 3 * 11 ** 2 * 10177 ** 2 * 859267 ** 2 * 52437899 ** 2 and R == Z ** 4 - Z ** 2 + 1
assert H == 0x396C8C005555E1568C00AAAB0000AAAB

FAMILIES = ("g1", "torsion", "torsion_plus_g1", "composite", "cleared", "x_on_curve", "x_off_curve", "sign_edge",
            "encoding")
MINIMUM = {"g1": 138, "torsion": 80, "torsion_plus_g1": 80, "composite": 24, "cleared": 16, "x_on_curve": 14,
           "x_off_curve": 69, "sign_edge": 8, "encoding": 10}


def draw(tag, mod):
    return int.from_bytes(hashlib.shake_256(f"{SEED}/{tag}".encode()).digest(64), "big") % mod


def sqrt_fp(a):
    """A square root of a, or None (p = 3 mod 4)."""
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def curve_point(tag):
    """A curve point with a uniformly drawn x (almost never in G1: the cofactor is ~2^126)."""
    for j in itertools.count():
        x = draw(f"{tag}/x{j}", P)
        y = sqrt_fp(x * x * x + 4)
        if y is not None:
            return (x, y if draw(f"{tag}/s{j}", 2) else P - y)


def g1_point(tag):
    return o.scalar_mul(draw(tag, R - 1) + 1, o.G1)


def record(x, sign=0, flags=0x80):
    b = bytearray(x.to_bytes(48, "big"))
    assert b[0] < 0x20
    b[0] |= flags | (0x20 if sign else 0)
    return bytes(b)


def expected(rec):
    """(status with the subgroup test, status without it, point or None) from the definitions."""
    comp, inf, sign = rec[0] & 0x80, rec[0] & 0x40, rec[0] & 0x20
    x = int.from_bytes(rec, "big") & ((1 << 381) - 1)
    if not comp:
        return BAD_ENCODING, BAD_ENCODING, None
    if inf:
        st = BAD_ENCODING if (sign or x) else INFINITY
        return st, st, None
    if x >= P:
        return BAD_ENCODING, BAD_ENCODING, None
    rhs = (x * x * x + 4) % P
    if pow(rhs, (P - 1) // 2, P) != 1:                                    # Euler (rhs = 0 has no point either)
        return NOT_ON_CURVE, NOT_ON_CURVE, None
    y = sqrt_fp(rhs)
    if (y > HALF) != bool(sign):
        y = P - y
    pt = (x, y)
    assert o.is_on_curve(pt) and o.compress(pt) == rec
    return (OK if o.scalar_mul(R, pt) is None else NOT_IN_SUBGROUP), OK, pt


@functools.lru_cache(maxsize=None)
def torsion_point(l, i):
    """The i-th point of order exactly l."""
    if l == 3:
        T = (0, 2) if i % 2 == 0 else (0, P - 2)                          # the only two: x^3 = 0
    else:
        for j in itertools.count():
            T = o.scalar_mul(H * R // (l * l), curve_point(f"torsion/{l}/{i}/{j}"))
            if T is not None:
                break
    assert o.is_on_curve(T) and o.scalar_mul(l, T) is None                # l prime and T != inf: order exactly l
    return T


@functools.lru_cache(maxsize=None)
def _sylow3():
    s, t = 0, P - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    n = 2
    while pow(n, (P - 1) // 3, P) == 1:
        n += 1
    g = pow(n, t, P)                                                       # generates the 3-Sylow subgroup, order 3^s
    return s, t, g


def cube_roots(a):
    """All x with x^3 == a (mod p): none or three."""
    a %= P
    if a == 0 or pow(a, (P - 1) // 3, P) != 1:
        return []
    s, t, g = _sylow3()
    e = pow(3, -1, t)
    c = pow(a, e, P)                                                       # c^3 = a * b with b = a^(3e - 1) in the 3-Sylow subgroup
    b = c * c * c * pow(a, -1, P) % P
    d = 1
    for _ in range(3 ** s):                                                # b is a cube in a cyclic group of 3^s elements: search
        if d * d * d % P == b:
            break
        d = d * g % P
    root = c * pow(d, -1, P) % P
    omega = pow(g, 3 ** (s - 1), P)
    roots = sorted({root, root * omega % P, root * omega * omega % P})
    assert len(roots) == 3 and all(pow(x, 3, P) == a for x in roots)
    return roots


@functools.lru_cache(maxsize=None)
def sign_edge_distances(count=4):
    """The first `count` d >= 0 for which y = (p - 1) / 2 - d has curve points."""
    out = []
    for d in itertools.count():
        y = HALF - d
        if cube_roots(y * y - 4):
            out.append(d)
            if len(out) == count:
                return tuple(out)


# --- the families: generators of (record, built-to-be status with the test, built-to-be point) ---
def fam_g1():
    for i in range(69):
        k = (1, 2, 3, R - 1, R - 2)[i] if i < 5 else draw(f"g1/{i}", R - 1) + 1
        pt = o.scalar_mul(k, o.G1)
        for q in (pt, o.neg(pt)):
            yield o.compress(q), OK, q


def fam_torsion():
    for l in PRIMES:
        for i in range(8):
            T = torsion_point(l, i)
            for q in (T, o.neg(T)):
                yield o.compress(q), NOT_IN_SUBGROUP, q


def fam_torsion_plus_g1():
    for l in PRIMES:
        for i in range(8):
            pt = o.add(torsion_point(l, i), g1_point(f"tq/{l}/{i}"))
            assert o.scalar_mul(R, pt) is not None
            for q in (pt, o.neg(pt)):
                yield o.compress(q), NOT_IN_SUBGROUP, q


def fam_composite():
    """[r] Q (order divides the cofactor, no G1 part) and T_l + T_l' of order l l'."""
    for i in range(4):
        pt = o.scalar_mul(R, curve_point(f"rq/{i}"))
        assert pt is not None and o.scalar_mul(H, pt) is None
        for q in (pt, o.neg(pt)):
            yield o.compress(q), NOT_IN_SUBGROUP, q
    for la, lb in ((3, 11), (10177, 52437899)):
        for i in range(4):
            pt = o.add(torsion_point(la, i), torsion_point(lb, i))
            assert o.scalar_mul(la, pt) is not None and o.scalar_mul(lb, pt) is not None
            assert o.scalar_mul(la * lb, pt) is None
            for q in (pt, o.neg(pt)):
                yield o.compress(q), NOT_IN_SUBGROUP, q


def fam_cleared():
    for i in range(8):
        pt = o.scalar_mul(H, curve_point(f"cleared/{i}"))
        assert pt is not None and o.scalar_mul(R, pt) is None
        for q in (pt, o.neg(pt)):
            yield o.compress(q), OK, q


def fam_x_on_curve():
    for x in (0, 4, 5, 6, P - 3, P - 8, P - 11):
        y = sqrt_fp(x * x * x + 4)
        assert y is not None, x
        for sign in (0, 1):
            yield record(x, sign), None, (x, y if (y > HALF) == bool(sign) else P - y)


def fam_x_off_curve():
    for x in (1, 2, 3, P - 1, P - 2):
        assert pow(x * x * x + 4, (P - 1) // 2, P) == P - 1, x
        for sign in (0, 1):
            yield record(x, sign), NOT_ON_CURVE, None
    for i in range(64):
        for j in itertools.count():
            x = draw(f"off/{i}/{j}", P)
            if pow(x * x * x + 4, (P - 1) // 2, P) == P - 1:
                break
        yield record(x, i & 1), NOT_ON_CURVE, None


def fam_sign_edge():
    for d in sign_edge_distances():
        y = HALF - d
        for x in cube_roots(y * y - 4):
            assert o.is_on_curve((x, y))
            yield record(x, 0), None, (x, y)                               # flag clear: the smaller root, d below the threshold
            yield record(x, 1), None, (x, P - y)                           # flag set: (p - 1) / 2 + 1 + d


def fam_encoding():
    yield record(P, 0), BAD_ENCODING, None                                 # x = p
    yield record(P + 1, 0), BAD_ENCODING, None
    yield record((1 << 381) - 1, 0), BAD_ENCODING, None
    yield record(o.GX, 0, flags=0), BAD_ENCODING, None                     # compression flag clear
    inf = o.compress(None)
    yield bytes([0xE0]) + inf[1:], BAD_ENCODING, None                      # infinity with the sign flag
    for pos in (0, 1, 24, 47):
        b = bytearray(inf)
        b[pos] |= 0x01
        yield bytes(b), BAD_ENCODING, None                                 # infinity with a stray bit
    yield inf, INFINITY, None


GENERATORS = {"g1": fam_g1, "torsion": fam_torsion, "torsion_plus_g1": fam_torsion_plus_g1, "composite": fam_composite,
              "cleared": fam_cleared, "x_on_curve": fam_x_on_curve, "x_off_curve": fam_x_off_curve,
              "sign_edge": fam_sign_edge, "encoding": fam_encoding}


def entries(family, count=None):
    """The first `count` entries of a family (all of them by default) as
    (record, status with the subgroup test, status without it, 96 point bytes)."""
    out = []
    for rec, built, built_pt in itertools.islice(GENERATORS[family](), count):
        st_sub, st_nosub, pt = expected(rec)
        assert built is None or built == st_sub, (family, rec.hex(), built, st_sub)
        assert built_pt == pt or (built_pt is None and st_sub in (INFINITY, BAD_ENCODING, NOT_ON_CURVE)), (family, rec.hex())
        assert st_nosub == (OK if st_sub == NOT_IN_SUBGROUP else st_sub)
        ptb = bytes(96) if pt is None else pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")
        out.append((rec, st_sub, st_nosub, ptb))
    return out


def arrays():
    recs, st_sub, st_nosub, pts, fam = [], [], [], [], []
    for name in FAMILIES:
        got = entries(name)
        assert len(got) >= MINIMUM[name], (name, len(got))
        print(f"{name:16s} {len(got):4d} records", flush=True)
        for rec, a, b, ptb in got:
            recs.append(np.frombuffer(rec, dtype=np.uint8))
            pts.append(np.frombuffer(ptb, dtype=np.uint8))
            st_sub.append(a)
            st_nosub.append(b)
            fam.append(name)
    return {"records": np.stack(recs), "status_subgroup": np.array(st_sub, dtype=np.uint8),
            "status_no_subgroup": np.array(st_nosub, dtype=np.uint8), "points": np.stack(pts),
            "family": np.array(fam, dtype="S16")}


def npz_bytes(arrs):
    """An .npz with nothing in it that changes between runs (stored, fixed timestamps)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrs.items():
            f = io.BytesIO()
            np.lib.format.write_array(f, np.ascontiguousarray(a), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, f.getvalue())
    return buf.getvalue()


def main():
    o.self_check()
    assert o.scalar_mul(3, (0, 2)) is None and o.is_on_curve((0, 2))
    print("p - 1 = 3^%d * t; sign-edge distances below (p - 1) / 2: %s" % (_sylow3()[0], list(sign_edge_distances())))
    data = npz_bytes(arrays())
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote", OUT, len(data), "bytes")


if __name__ == "__main__":
    main()
