"""The big-integer model of the division-step inversion (tests/fp_divsteps_model.py) on its case families.  The model
asserts at every batch that the divisions by 2^30 are exact, the matrix bound, |f|, |g| < 2^381 and d, e in (-2p, p),
and at the end g = 0 and f = +-1; here its result is compared with pow(x, p - 2, p), the step at which g became 0 with
the paper's bound, and the two entry forms (repackings and Montgomery constants) with the inverse in their own radix.
This is the argument the header's other tests rest on: they compare the header with this model bit for bit."""
import fp_divsteps_model as m

P = m.P


def test_constants():
    assert m.STEPS == 1110 and m.BOUND == 1101 and m.STEPS >= m.BOUND
    assert m.PINV30 * P % (1 << 30) == 1
    assert m.K28 == pow(2, 3 * 392, P) and m.KGNARK == pow(2, 2 * 384 + 392, P)


def test_body_on_every_case_family():
    cases = m.all_cases()
    assert len(cases) == 9 + 2 * len(m.EDGE_KS) + 64 + 1000
    for x in cases:
        y, viol = m.invert_body(x)  # asserts the per-batch invariants
        assert viol == 0, hex(x)
        assert y == pow(x, P - 2, P), hex(x)
    assert m.invert_body(0) == (0, 0)


def test_step_counts():
    longest = m.longest_cases()
    steps = [m.first_zero_step(x) for x in m.fixed_cases() + m.random_cases()] + [n for _, n in longest]
    print("steps until g = 0: max", max(steps), "the 64 longest of 20,000:", longest[-1][1], "...", longest[0][1])
    assert max(steps) <= m.BOUND
    assert max(steps) > 780  # the late batches are exercised
    assert all(n == m.first_zero_step(x) for x, n in longest[:4])


def test_repackings_round_trip():
    for v in m.fixed_cases() + m.random_cases(50):
        l28 = m.limbs28(v)
        l30 = m.repack(l28, 28, 30, 13)
        assert m.value(l30, 30) == v and all(l < 1 << 30 for l in l30)
        assert m.repack(l30, 30, 28, 14) == l28
        l32 = m.limbs(v, 32, 12)
        assert m.repack(m.repack(l32, 32, 30, 13), 30, 32, 12) == l32


def test_raw_form():
    """invert_ds(F28&, const F28&): any normalised a < 2p in, the Montgomery form of the inverse out, below 2p."""
    for a in m.all_cases()[:200] + list(m.RAW_EXTRA) + [c + P for c in m.fixed_cases() if c + P < 2 * P]:
        y, viol = m.invert_raw28(a)
        assert viol == 0 and y < 2 * P
        assert y % P == m.want_raw28(a % P), hex(a)
    assert m.invert_raw28(P) == (0, 0) and m.invert_raw28(0) == (0, 0)


def test_gnark_form():
    for a in m.all_cases()[:200]:
        y, viol = m.invert_gnark(a)
        assert viol == 0 and y == m.want_gnark(a), hex(a)
    assert m.invert_gnark(0) == (0, 0)
    # the Montgomery one is its own inverse
    assert m.invert_gnark(m.R384 % P) == (m.R384 % P, 0)
