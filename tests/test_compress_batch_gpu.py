"""curdle_g1_compress_batch / _device on the GPU (compress_kernels.hip): every encoding equals curdle_g1_compress of
the same G1Jac value (host code) and oracle.compress of the point it stands for.  The kernel runs one lane per point
under ONE launch rule (blocks of 256 at every size), so the sizes straddle a wave (64) and a block (256) of lanes, and
the quads' 16 of the other point kernels besides."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000]


def jac_limbs(oracle, pt, z):
    """The Jacobian representative (x z^2, y z^3, z) of an affine point, as gnark limbs; X and Y as given when z = 0."""
    P = oracle.P
    if pt is None:
        pt, z = (5, 7), 0
    x, y = pt
    if z:
        x, y = x * z * z % P, y * z * z * z % P
    return oracle.fp_to_mont_limbs(x) + oracle.fp_to_mont_limbs(y) + oracle.fp_to_mont_limbs(z)


def sqrt_or_none(oracle, x):
    P = oracle.P
    rhs = (x * x * x + 4) % P
    y = pow(rhs, (P + 1) // 4, P)
    return y if y * y % P == rhs else None


@pytest.fixture(scope="module")
def pool(gpu, oracle):
    """Distinct affine points (None = infinity): multiples of G, P beside -P, and curve points whose x has its top bits
    set (x just below p; the encoding says nothing about the subgroup and neither does the kernel)."""
    rand = oracle.Rand(4242)
    pts = []
    for _ in range(12):
        p = oracle.scalar_mul(rand.get_fr(), oracle.G1)
        pts += [p, oracle.neg(p)]
    x = oracle.P - 1
    while len(pts) < 30:
        y = sqrt_or_none(oracle, x)
        if y is not None:
            pts += [(x, y), (x, oracle.P - y)]
        x -= 1
    assert {oracle.compress(p)[0] >> 5 for p in pts} == {0b100, 0b101}          # both sign flags
    assert sum(1 for p in pts if p[0] >> 376 == oracle.P >> 376) >= 6           # x with the top byte of p
    return pts


def batch(oracle, pool, n, seed, inf_at=()):
    """n Jacobian points over the pool: Z = 1, random Z and Z = 0 (with non-zero X, Y) in turn; returns the limbs and
    the expected encodings."""
    rng = np.random.default_rng(seed)
    limbs, want = [], []
    for i in range(n):
        pt = pool[i % len(pool)] if n > 1 else pool[seed % len(pool)]
        mode = (i // len(pool) + i) % 3
        if i in inf_at:
            pt = None
        z = 1 if mode == 0 else int.from_bytes(rng.bytes(47), "big") + 2
        limbs.append(jac_limbs(oracle, pt, z))
        want.append(oracle.compress(pt))
    return np.array(limbs, dtype=np.uint64), want


def check(gpu, got, limbs, want):
    assert got.shape == (len(want), 48) and got.dtype == np.uint8
    for i, w in enumerate(want):
        assert got[i].tobytes() == w, i
    # ... and the host's single call on the same limbs (every point below 64, then a sample)
    idx = list(range(min(64, len(want)))) + list(range(64, len(want), 37))
    for i in idx:
        assert gpu.g1_compress(limbs[i]) == want[i], i


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, oracle, pool, n):
    inf_at = {0, n // 2, n - 1} if n >= 15 else ()
    limbs, want = batch(oracle, pool, n, n, inf_at)
    check(gpu, gpu.g1_compress_batch(limbs), limbs, want)


def test_infinity_takes_no_neighbour_with_it(gpu, oracle, pool):
    """Z = 0 with non-zero X and Y at the start, in runs in the middle and at the end; then nothing but infinity."""
    n = 70
    inf_at = {0, 1, 30, 31, 32, 33, 63, 64, 68, 69}
    limbs, want = batch(oracle, pool, n, 9, inf_at)
    assert limbs[30, :12].any()                                                # X, Y are not zero there
    check(gpu, gpu.g1_compress_batch(limbs), limbs, want)
    limbs, want = batch(oracle, pool, 65, 10, set(range(65)))
    assert set(want) == {bytes([0xC0]) + bytes(47)}
    check(gpu, gpu.g1_compress_batch(limbs), limbs, want)


def test_resident_points_on_a_callers_stream(gpu, oracle, pool):
    """The points are written on the caller's stream immediately before the call, which reads them in that order."""
    import torch
    limbs, want = batch(oracle, pool, 300, 21, {7})
    src = torch.from_numpy(limbs.view(np.int64)).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_in = torch.zeros_like(src, device="cuda:0")
        d_out = torch.zeros(300 * 48, dtype=torch.uint8, device="cuda:0")
        d_in.copy_(src, non_blocking=True)
        gpu.g1_compress_batch_device(d_in.data_ptr(), 300, d_out.data_ptr(), stream=s.cuda_stream)
        got = d_out.cpu().numpy().reshape(300, 48)
    check(gpu, got, limbs, want)
    # ... and on the library's own stream
    torch.cuda.synchronize()
    d_out.zero_()
    torch.cuda.synchronize()
    gpu.g1_compress_batch_device(d_in.data_ptr(), 300, d_out.data_ptr())
    check(gpu, d_out.cpu().numpy().reshape(300, 48), limbs, want)


@pytest.mark.parametrize("off_in,off_out", [(1, 0), (0, 3), (5, 7), (8, 2)])
def test_device_pointers_of_any_alignment(gpu, oracle, pool, off_in, off_out):
    import torch
    n = 67
    limbs, want = batch(oracle, pool, n, 33 + off_in, {n - 1})
    raw = np.zeros(n * 144 + 16, dtype=np.uint8)
    raw[off_in: off_in + n * 144] = limbs.view(np.uint8).reshape(-1)
    d_in = torch.from_numpy(raw).to("cuda:0")
    d_out = torch.full((n * 48 + 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    gpu.g1_compress_batch_device(d_in.data_ptr() + off_in, n, d_out.data_ptr() + off_out)
    out = d_out.cpu().numpy()
    check(gpu, out[off_out: off_out + n * 48].reshape(n, 48), limbs, want)
    assert (out[:off_out] == 0x5A).all() and (out[off_out + n * 48:] == 0x5A).all()     # nothing beyond the n x 48 bytes


def sign_edge_case(oracle):
    """The records of tests/golden/decode_edge_records.npz that pin the sign flag, each beside the affine point it
    stands for: every record of the sign_edge and x_on_curve families and the order-3 points (0, +-2) of torsion.  The
    record IS the expected encoding; nothing of this project computed it.  Every point comes as G1Jac with Z = 1,
    Z = p - 1 and a seeded random Z.  Returns (limbs (3 k, 18), the 3 k records)."""
    import os
    from conftest import ROOT
    z = np.load(os.path.join(ROOT, "tests", "golden", "decode_edge_records.npz"))
    P, half = oracle.P, (oracle.P - 1) // 2
    rng = np.random.default_rng(381)
    limbs, want, near = [], [], set()
    for fam, rec, ptb in zip(z["family"], z["records"], z["points"]):
        b = ptb.tobytes()
        pt = (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))
        if not (fam in (b"sign_edge", b"x_on_curve") or (fam == b"torsion" and pt[0] == 0)):
            continue
        assert oracle.is_on_curve(pt) and pt[1] != half
        for zc in (1, P - 1, int.from_bytes(rng.bytes(47), "big") + 2):
            limbs.append(jac_limbs(oracle, pt, zc))
            want.append(rec.tobytes())
        if fam == b"sign_edge":
            # what the family was built to be: y and (p - 1) / 2 differ in the lowest 32-bit word alone
            assert pt[1] >> 32 == half >> 32
            assert bool(rec[0] & 0x20) == (pt[1] > half)
            near.add(int(rec[0]) & 0x20)
    assert near == {0, 0x20}                                                    # both flags at the threshold
    assert {w[0] for w in want if w[1:] == bytes(47)} == {0x80, 0xA0}           # ... and at x = 0
    assert len(want) == 3 * (24 + 14 + 16)                                      # torsion holds (0, 2) and (0, -2) eight times each
    return np.array(limbs, dtype=np.uint64), want


def test_sign_edges_from_the_decode_fixture(gpu, oracle):
    """y within 15 of (p - 1) / 2 on either side: only here can the low eleven words of the kernel's own copy of
    (p - 1) / 2 change an output byte (the decoder's copy is pinned by the same records in test_decode_edges_gpu)."""
    limbs, want = sign_edge_case(oracle)
    got = gpu.g1_compress_batch(limbs)
    assert got.shape == (len(want), 48) and got.dtype == np.uint8
    for i, w in enumerate(want):
        assert got[i].tobytes() == w, i
        assert gpu.g1_compress(limbs[i]) == w, i


def test_round_trip_through_the_decoder(gpu, oracle, pool):
    """decompress_batch(compress_batch(P)) == P for subgroup points and infinity."""
    pts = pool[:24] + [None]
    limbs = np.array([jac_limbs(oracle, p, 3 + i) for i, p in enumerate(pts)], dtype=np.uint64)
    enc = gpu.g1_compress_batch(limbs)
    aff, st = gpu.g1_decompress_batch(enc.tobytes())
    assert st.tolist() == [gpu.DECODE_OK] * 24 + [gpu.DECODE_INFINITY]
    for i, p in enumerate(pts):
        assert aff[i].tolist() == oracle.affine_to_mont_limbs(p), i
