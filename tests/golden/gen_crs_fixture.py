#!/usr/bin/env python3
"""Generates tests/golden/crs_ell4.bin: a CRS of ell = 4 in the library's wire form (include/curdle_msm.h: Gs, Hs, H, Gt,
Gu, Gsum, Hsum, each point in gnark's 48-byte compressed encoding, 48 (ell + 9) = 624 bytes) that NO common.Rand seed
produces: every generator is s * G for a scalar written below, and the two sums are the oracle's sequential additions.

Every byte comes from the pure-Python oracle (oracle/py/bls12381_ref.py: scalar_mul, add, compress), never from this
project's library, so curdle_crs_from_bytes is pinned against an independent encoder and not only against
curdle_crs_to_bytes.

Run:  python tests/golden/gen_crs_fixture.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "py"))
import bls12381_ref as o  # noqa: E402

OUT = os.path.join(HERE, "crs_ell4.bin")
ELL = 4
N_BLINDERS = 4

# The discrete logarithms of the eleven generators to the base G, in wire order.  Fixed by hand; distinct, non-zero, below r.
GS_SCALARS = (
    0x1b2f0c6a59d3e8471f0a6c25b94d7e3810f2a6c4e9b1d7053a8c6e2f4b1907,
    0x02e4a91c7d3b5f6081a2c4e6f8091b3d5f7a9cbe0d2f416385a7c9eb0d2f41,
    0x5c0ffee15bad5eed0ddba11c0dec0de5ca1ab1e5a11ab0a7d0d0fa11f00d42,
    0x3141592653589793238462643383279502884197169399375105820974944b,
)
HS_SCALARS = (
    0x2718281828459045235360287471352662497757247093699959574966967a,
    0x1618033988749894848204586834365638117720309179805762862135448c,
    0x14142135623730950488016887242096980785696718753769480731766797,
    0x17320508075688772935274463415058723669428052538103806280558069,
)
H_SCALAR = 0x6a09e667f3bcc908b2fb1366ea957d3e3adec17512775099da2f590b066732
GT_SCALAR = 0x3c6ef372fe94f82be73980c0b9db90681d3a5c1f0e9b7d245f6a8c3e1b0975
GU_SCALAR = 0x510e527fade682d19b05688c2b3e6c1f1f83d9abfb41bd6b5be0cd19137e21


def crs_points():
    """The seven fields as oracle affine points: (Gs, Hs, H, Gt, Gu, Gsum, Hsum)."""
    scalars = GS_SCALARS + HS_SCALARS + (H_SCALAR, GT_SCALAR, GU_SCALAR)
    assert len(GS_SCALARS) == ELL and len(HS_SCALARS) == N_BLINDERS
    assert len(set(scalars)) == len(scalars) and all(0 < s < o.R for s in scalars)
    Gs = [o.scalar_mul(s, o.G1) for s in GS_SCALARS]
    Hs = [o.scalar_mul(s, o.G1) for s in HS_SCALARS]
    H, Gt, Gu = (o.scalar_mul(s, o.G1) for s in (H_SCALAR, GT_SCALAR, GU_SCALAR))
    Gsum, Hsum = o.INF, o.INF
    for g in Gs:                                   # crs.go:41-48: sequential additions
        Gsum = o.add(Gsum, g)
    for h in Hs:
        Hsum = o.add(Hsum, h)
    assert Gsum == o.scalar_mul(sum(GS_SCALARS) % o.R, o.G1) and Hsum == o.scalar_mul(sum(HS_SCALARS) % o.R, o.G1)
    return Gs, Hs, H, Gt, Gu, Gsum, Hsum


def wire_bytes() -> bytes:
    Gs, Hs, H, Gt, Gu, Gsum, Hsum = crs_points()
    data = b"".join(o.compress(p) for p in Gs + Hs + [H, Gt, Gu, Gsum, Hsum])
    assert len(data) == 48 * (ELL + 9) == 624
    return data


def main():
    o.self_check()
    data = wire_bytes()
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote", OUT, len(data), "bytes")


if __name__ == "__main__":
    main()
