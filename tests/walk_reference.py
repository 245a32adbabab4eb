"""Exact closed form of an MSM over the known-discrete-log walk, vectorised so that it scales to 2^27 pairs.

The walk P_i = (k + i q) G (curdle_synth_points_walk_device) makes any MSM over it one scalar multiple of G:
    sum_i s_(a+i) P_(a+i) = ((k + a q) * sum s_i + q * sum i s_i) G
for a slice that starts at index a of the walk.  Both sums are taken over the scalars' MONTGOMERY words m_i, exactly,
with numpy: each 64-bit word is split into 16-bit pieces, the pieces are summed in blocks short enough that every
partial is an integer below 2^53 (exact in the float64 product that sums them), and the block totals are carried in
Python integers.  canonical = m * R^-1 (mod r) is linear,
so one multiplication by R^-1 per sum converts them.  (The per-row form with Python integers, _walk_expected in
tests/test_msm_gpu.py, is minutes of work at 2^27.)"""
import numpy as np

_BLOCK = 1 << 20  # rows per block: piece < 2^16, row index < 2^20 (see mont_sums)


def mont_sums(sc, block=_BLOCK):
    """(sum m_i, sum i * m_i) over the Montgomery integers m_i of uint64[n, 4] scalar words, as Python integers.
    Nothing is reduced: the words may be any 256-bit values."""
    sc = np.ascontiguousarray(sc, dtype=np.uint64)
    assert sc.ndim == 2 and sc.shape[1] == 4, sc.shape
    assert 1 <= block <= _BLOCK
    s0 = s1 = 0
    for lo in range(0, len(sc), block):
        # little-endian words: column 4 w + t of the uint16 view is bits [16 t, 16 t + 16) of word w, weight 2^(16 (4 w + t))
        pieces = sc[lo:lo + block].view(np.uint16).reshape(-1, 16).astype(np.float64)
        # one float64 product for all three weightings (1, the row index's low and high 10 bits): every product and
        # partial sum is an integer below 2^20 * 2^16 * 2^10 = 2^46, exact in a double
        rows = np.arange(len(pieces), dtype=np.int64)
        weights = np.stack([np.ones(len(pieces)), (rows & 1023).astype(np.float64), (rows >> 10).astype(np.float64)])
        col = weights @ pieces
        assert col.max() < 2.0 ** 53
        col = col.astype(np.uint64)
        b0 = sum(int(v) << (16 * c) for c, v in enumerate(col[0]))
        b1 = sum((int(v) + (int(h) << 10)) << (16 * c) for c, (v, h) in enumerate(zip(col[1], col[2])))
        s0 += b0
        s1 += b1 + lo * b0                            # row lo + j of the whole array is row j of the block
    return s0, s1


def walk_exponent(oracle, k, q, sc, start=0, block=_BLOCK):
    """e with MSM(P_start .. P_(start + n - 1); sc) = e G, reduced mod r."""
    m0, m1 = mont_sums(sc, block)
    s0 = m0 * oracle.R_FR_INV % oracle.R
    s1 = m1 * oracle.R_FR_INV % oracle.R
    return ((k + start * q) * s0 + q * s1) % oracle.R


def walk_expected(oracle, coracle, k, q, sc, start=0):
    """The MSM over the walk's pairs [start, start + n) as the library returns it (canonical Jacobian, Montgomery limbs)."""
    aff = coracle.scalar_mul_gen(walk_exponent(oracle, k, q, sc, start))
    pt = oracle.affine_from_mont_limbs([int(v) for v in aff])
    return np.array(oracle.jac_to_mont_limbs(pt), dtype=np.uint64)
