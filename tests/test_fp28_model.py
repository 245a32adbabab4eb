"""The executable model of the device field layer (tests/fp28_model.py) without a GPU: its constants are the
header's, its products are Montgomery products in plain big integers, its generators reach the bounds they
claim, and a representation just past each bound trips its assertion -- so the GPU tests that compare the
device words with the model's (tests/test_fp28_bounds_gpu.py) test the layer at its edges."""
import random

import numpy as np
import pytest

import fp28_model as m

P = m.P


def test_constants_are_the_headers():
    T = m.header_tables()
    assert m.value1(T["kP"]) == P and m.N0 == 0x0FFCFFFD and (m.N0 * P) % (1 << 28) == (1 << 28) - 1
    assert m.value1(T["kOne"]) == m.RP % P
    assert m.value1(T["kToInt"]) == (1 << 400) % P
    assert m.value1(T["kToExt"]) == (1 << 384) % P
    assert m.value1(T["kToExtX16"]) == (1 << 388) % P
    assert m.value1(T["kToExtY64"]) == (1 << 390) % P
    beta = m.from_mont(m.value1(T["kBeta"]))
    assert beta != 1 and pow(beta, 3, P) == 1
    for name in ("kP", "kOne", "kToInt", "kToExt", "kToExtX16", "kToExtY64", "kBeta"):
        assert all(x <= m.MASK for x in T[name][:13]) and m.value1(T[name]) <= P, name
    for K in (4, 8, 16):                      # K p, limbs 0..12 >= 2^28 - 1, limb 13 = top(K p) - 1
        L = T[f"kK{K}"]
        assert m.value1(L) == K * P
        assert all((1 << 28) - 1 <= x < 1 << 30 for x in L[:13]) and L[13] == m.limbs_of(K * P)[13] - 1
    L = T["kK8B"]                             # 8p, limbs 0..12 >= 2^30 - 4
    assert m.value1(L) == 8 * P and all((1 << 30) - 4 <= x < 1 << 31 for x in L[:13])


def _families(K, cap_bits=30, n_random=200, seed=0):
    rnd = random.Random(seed)
    vals = [0, 1, P - 1, P, P + 1, 2 * P - 1, K * P - 1] + [m.top_below(rnd.randrange(P), K) for _ in range(8)]
    vals = [v for v in vals if v < K * P]
    out = [m.limbs_of(v) for v in vals] + [m.push_limbs(v, cap_bits) for v in vals]
    out.append(m.low_limbs_at(0))
    out += m.rand_reps([rnd.randrange(K * P) for _ in range(n_random)], 1 << cap_bits,
                       np.random.default_rng(seed)).tolist()
    return m.rows(out)


def _check_product(r, exact):
    for got, x in zip(m.value(r), exact):
        mm = (-x * pow(P, -1, m.RP)) % m.RP
        assert got == (x + mm * P) >> 392                 # the very words of (x + m p) / 2^392
        assert got % P == x * m.RP_INV % P and got < 2 * P
    assert m.normalised(r).all()


def test_products_are_montgomery_products_for_every_family():
    a = _families(32)
    b = a[::-1].copy()
    _check_product(m.mul(a, b), [x * y for x, y in zip(m.value(a), m.value(b))])
    _check_product(m.sqr(a), [x * x for x in m.value(a)])
    s = m.isqrt_below(m.RP * P)                          # the largest square below 2^392 p
    _check_product(m.sqr(m.rows([m.push_limbs(s)])), [s * s])
    y = 32 * P - 1
    x = (m.RP * P - 1) // y                               # the largest a*b below 2^392 p
    _check_product(m.mul(m.arr([x]), m.arr([y])), [x * y])
    # mul2_inl as madd calls it: R and Q - X3 are sub_raw<16> results, 16p - Y1, PPP normalised
    n = 64
    r = m.sub_raw(16, m.arr([2 * P - 1] * n), m.arr([15 * P - 1 - i for i in range(n)]))
    q = m.sub_raw(16, m.arr([2 * P - 1 - i for i in range(n)]), m.arr([10 * P - 1] * n))
    ny = m.sub_raw(16, m.zeros(n), m.arr([i for i in range(n)]))
    ppp = m.arr([2 * P - 1 - i for i in range(n)])
    _check_product(m.mul2(r, q, ny, ppp), [w * x + y * z for w, x, y, z in
                                           zip(m.value(r), m.value(q), m.value(ny), m.value(ppp))])


def test_generators_meet_their_claims():
    rng = np.random.default_rng(3)
    for K in (2, 4, 10, 16, 32):
        for v in (0, 1, P - 1, 12345):
            t = m.top_below(v, K)
            assert t < K * P <= t + P and t % P == v % P
            for cap in (29, 30):
                L = m.push_limbs(t, cap)
                assert m.value1(L) == t and max(L[:13]) < 1 << cap and max(L[:13]) >= (1 << cap) - (1 << 28)
    y = m.arr([0, 1, P - 1, 2 * P - 1])
    ny = m.neg_words(y)
    assert [4 * P - v for v in m.value(y)] == m.value(ny) and (ny < (1 << 30)).all()
    reps = m.rand_reps([P - 1] * 100, int(2 ** 29.6), rng)
    assert set(m.value(reps)) == {P - 1} and (reps.astype(float) < 2 ** 29.6).all()


def test_accumulator_margins_at_the_extremes(capsys):
    """The largest column accumulator the bounds allow, against 2^64 (fp28.h's 14 * 2^60 + 14 * 2^56 budget;
    gen_mac.py's "<= 29 products"): every limb of both factors at 2^30 - 1, and mul2_inl with each leg at
    its limit."""
    m.STATS.clear()
    top = m.low_limbs_at(0)                               # limbs 0..12 at 2^30 - 1
    a = m.rows([top])
    m.mul(a, a)
    m.sqr(a)
    c296, c292 = int(2 ** 29.6) - 1, int(2 ** 29.2) - 1
    m.mul2(a, m.rows([[c296] * 13 + [0]]), m.rows([[c292] * 13 + [0]]), m.rows([[m.MASK] * 13 + [0]]))
    for k, v in sorted(m.STATS.items()):
        assert v < 1 << 64
        with capsys.disabled():
            print(f"\n{k}: peak column accumulator {v / 2 ** 64:.4f} of 2^64", end="")
    assert m.STATS["mul_inl"] > 0.8 * 2 ** 64              # the families really drive the columns
    assert m.STATS["mul2_inl"] > 0.7 * 2 ** 64


def test_just_past_each_bound_trips_the_model():
    n1 = m.rows([m.low_limbs_at(0)])
    over = m.rows([[1 << 30] + [0] * 13])
    with pytest.raises(m.ContractError, match="2\\^30"):
        m.mul(over, n1)
    y = 32 * P - 1
    x = (m.RP * P) // y + 1                              # a*b just at / above 2^392 p
    with pytest.raises(m.ContractError, match="2\\^392"):
        m.mul(m.arr([x]), m.arr([y]))
    # past the contract the product leaves its promise (r < 2p) ...
    r = m.mont([(m.arr([x * 4]), m.arr([y]))])
    assert m.value1(r[0]) >= 2 * P
    # ... and limbs a fifth of a bit above 2^30 overflow a column accumulator
    wide = m.rows([[int(2 ** 30.2)] * 13 + [0]])
    with pytest.raises(m.OverflowError_, match="2\\^64"):
        m.mont([(wide, wide)])
    with pytest.raises(m.OverflowError_, match="cross"):
        m.sqr(m.rows([[int(2 ** 30.6)] * 13 + [0]]), contract=False)   # a square's doubled cross sum
    c296, c292 = int(2 ** 29.6) + 1, int(2 ** 29.2) + 1
    with pytest.raises(m.ContractError, match="both"):
        m.mul2(m.rows([[c296] + [0] * 13]), m.rows([[c296] + [0] * 13]), m.zeros(1), m.zeros(1))
    with pytest.raises(m.ContractError, match="2\\^29.2"):
        m.mul2(n1, m.zeros(1), m.rows([[c292] + [0] * 13]), m.zeros(1))
    for K in (4, 8, 16):
        m.sub_raw(K, m.zeros(1), m.arr([(K - 1) * P - 1]))
        with pytest.raises(m.ContractError, match=f"below {K - 1}p"):
            m.sub_raw(K, m.zeros(1), m.arr([(K - 1) * P]))
    m.x3_fused(m.arr([2 * P - 1]), m.zeros(1), m.zeros(1))
    with pytest.raises(m.ContractError, match="q not normalised below 2p"):
        m.x3_fused(m.zeros(1), m.zeros(1), m.arr([2 * P]))
    # madd's y2 < 4p, and 8p - y as a negation would be past it (k_accumulate negates with sub_raw<4>)
    acc = (m.arr([9 * P]), m.arr([5 * P]), m.one(1), m.one(1))
    x2 = m.arr([P + 5])
    with pytest.raises(m.ContractError, match="y2"):
        m.madd(acc, x2, m.sub_raw(8, m.zeros(1), m.arr([1])))
    with pytest.raises(m.ContractError, match="y1"):
        m.dbl_affine(x2, m.arr([4 * P]))
    # a stored Y of 10p - 1 is accepted by every formula, and each of them gives Y < 6p back
    pt = (m.arr([10 * P - 1]), m.arr([10 * P - 1]), m.one(1), m.one(1))
    for out in (m.dbl(pt), m.add_pts(pt, (m.arr([P + 7]), m.arr([3]), m.one(1), m.one(1)))):
        m.check_stored(out, "Y up to 10p in")
    with pytest.raises(m.OverflowError_, match="stored Y"):
        m.check_stored(pt, "stored")
