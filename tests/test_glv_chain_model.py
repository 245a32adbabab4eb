"""tests/glv_chain_model.py, the scalar-domain model of the GLV chains on quads, on the CPU: its eigenvalue against
the kernels' beta, its classes against real points of the curve (part a), the single chain's freedom from exceptional
additions (part b), and the committed tracker members (tests/golden/tracker_chain_cases.npz) against the host build
of the split.  The GPU halves are tests/test_tracker_chain_events_gpu.py and tests/test_scalar_mul_special_gpu.py."""
import os
import sys

import numpy as np
import pytest

import glv_chain_model as M

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_tracker_chain_cases as gen  # noqa: E402

R, LAM = M.R, M.LAMBDA


def kernel_beta():
    """d28::kBeta of fp28.h (beta 2^392 mod p on 14 limbs of 28 bits), as an integer."""
    import fp28_model
    limbs = fp28_model.header_tables()["kBeta"]
    assert len(limbs) == 14
    return fp28_model.from_mont(sum(v << (28 * j) for j, v in enumerate(limbs)))


def phi(beta, pt):
    return None if pt is None else (beta * pt[0] % M_P, pt[1])


M_P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB


def test_lambda_is_the_eigenvalue_of_the_kernels_beta(cm, oracle):
    """The model's lambda is the one the kernels' phi(x, y) = (beta x, y) multiplies by, not its conjugate
    lambda^2; it is the lambda of tests/test_abi.py and the one operation 11 splits over."""
    import test_abi
    assert oracle.P == M_P and oracle.R == R and LAM == test_abi.GLV_LAMBDA
    assert (LAM * LAM + LAM + 1) % R == 0
    beta = kernel_beta()
    assert beta != 1 and pow(beta, 3, M_P) == 1
    for pt in (oracle.G1, oracle.scalar_mul(0xC0FFEE, oracle.G1)):
        assert phi(beta, pt) == oracle.scalar_mul(LAM, pt)
        assert phi(beta, pt) != oracle.scalar_mul(LAM * LAM % R, pt)
    vals = M.special_scalars()
    for v, (a, b, sa, sb) in zip(vals, M.splits(cm, vals, False)):
        assert (sa * a + sb * b * LAM - v) % R == 0, hex(v)


def test_the_scalar_with_the_largest_half(cm, oracle):
    """LARGEST_HALF_SCALAR is what tests/test_abi.py test_the_c_split_routine_against_big_integer_division finds:
    no case of it has a larger half."""
    import test_abi
    vals = test_abi.glv_split_cases(R, 300_000, 11)
    out = cm.selftest_op(11, test_abi.scalars_as_words(vals), False).astype(object)
    a = sum(out[:, j] << (32 * j) for j in range(4))
    b = sum(out[:, 4 + j] << (32 * j) for j in range(4))
    worst = max(int(a.max()), int(b.max()))
    at = [vals[i] for i in np.nonzero((a == worst) | (b == worst))[0]]
    assert M.LARGEST_HALF_SCALAR in at
    assert worst == (LAM + 1) // 2 and M.LARGEST_HALF_SCALAR in M.special_scalars()


# ------------------------------------------------------------------------------------------ part (a) ---
def point_trace(oracle, beta, tables, T=None):
    """The kernel's chain on real points: tables [(site, split, point)], the final addition of -T when T is
    given (False: T is infinity and nothing is added, as the kernel skips it).  [(bit, site, class)], acc."""
    def classify(acc, p):
        if p is None:
            return M.ADDS_INF
        if acc is None:
            return M.INTO_INF
        if acc == p:
            return M.EQUAL
        if acc == oracle.neg(p):
            return M.OPPOSITE
        return M.PLAIN

    built = []
    for site, (a, b, sa, sb), pt in tables:
        p1 = pt if sa > 0 else oracle.neg(pt)
        p2 = phi(beta, pt) if sb > 0 else oracle.neg(phi(beta, pt))
        built.append((site, a, b, (None, p1, p2, oracle.add(p1, p2))))       # glv_quad.h table: p3 = p1 + p2
    events, acc = [], None
    for bit in range(M.BITS - 1, -1, -1):
        acc = oracle.add(acc, acc)
        for site, a, b, tab in built:
            idx = ((a >> bit) & 1) | (((b >> bit) & 1) << 1)
            if idx:
                events.append((bit, site, classify(acc, tab[idx])))
                acc = oracle.add(acc, tab[idx])
    if T is not None:
        events.append((M.FINAL_BIT, M.SITE_T, classify(acc, oracle.neg(T) if T else None)))
    return events, acc


def joint_cases():
    """(s, c, k): 200 random triples, every k of the tracker search with random s and c, and for every such k pairs
    (s, c) built from one small s0 = a + b lambda whose leading bit pair stands alone (two clear pairs below it),
    so that c = +-s0, +-2 s0 against s = s0, 2 s0 line the two tables up by zero or one bit."""
    rng = np.random.default_rng(127)
    fr = lambda: int.from_bytes(rng.bytes(32), "big") % R  # noqa: E731
    cases = [(fr(), fr(), fr()) for _ in range(200)]
    for k in M.TRACKER_KS:
        cases += [(fr(), fr(), k) for _ in range(2)]
        a = (1 << 119) + int.from_bytes(rng.bytes(14), "big")           # 112 random bits below bits 118, 117
        b = int.from_bytes(rng.bytes(14), "big")
        s0 = (a + b * LAM) % R
        for s in (s0, 2 * s0):
            for c in (s0, R - s0, 2 * s0, R - 2 * s0):
                cases.append((s, c, k))
    return cases


def test_the_model_against_the_curve(cm, oracle, coracle):
    """Part (a): the model's step sequence replayed with the oracle's additions on real points -- its class at
    every step is what the points say, its final u P is the chain's sum and equals s P + c k P; on G and on a second
    point, with P at infinity for a few.  The built cases reach every class at both sites."""
    def c_mul(points, scalars):
        pts = np.array([oracle.affine_to_mont_limbs(p) for p in points], dtype=np.uint64)
        sc = np.array([oracle.fr_to_mont_limbs(v) for v in scalars], dtype=np.uint64)
        return oracle.jac_from_mont_limbs([int(v) for v in coracle.msm_naive(pts, sc)])

    beta = kernel_beta()
    cases = joint_cases()
    flat = [v for s, c, _ in cases for v in (s, c)]
    sp = M.splits(cm, flat, False)
    P2 = oracle.scalar_mul(0xC0FFEE, oracle.G1)
    seen = set()
    for j, (s, c, k) in enumerate(cases):
        P = None if j % 67 == 66 else (oracle.G1 if j % 2 else P2)
        Q, want = c_mul([P], [k]), c_mul([P, P], [s, c * k % R])     # the C oracle: s P + (c k) P, term by term
        t = (s + c * k) % R
        events, u = M.joint_chain(sp[2 * j], sp[2 * j + 1], k, t=t, p_is_infinity=P is None)
        got, acc = point_trace(oracle, beta, [(M.SITE_S, sp[2 * j], P), (M.SITE_C, sp[2 * j + 1], Q)], T=want or False)
        assert got == events, (j, hex(s), hex(c), hex(k))
        assert acc == want and (P is None or u == t), j
        if j % 16 == 0:
            assert oracle.scalar_mul(u, P) == acc, j
        assert events[-1][2] == (M.ADDS_INF if want is None else M.OPPOSITE)
        seen |= {(site, cls) for _, site, cls in events}
    for site in (M.SITE_S, M.SITE_C):
        for cls in (M.PLAIN, M.EQUAL, M.OPPOSITE, M.INTO_INF, M.ADDS_INF):
            assert (site, cls) in seen, (site, cls)


# ------------------------------------------------------------------------------------------ part (b) ---
def test_the_single_chain_meets_no_exceptional_addition(cm, oracle):
    """Part (b): over the special scalars and 100,000 random canonical ones the chain of k_scalar_mul_batch_quad
    holds no `equal` and no `opposite` step and ends on the scalar -- the lattice argument of
    tests/glv_chain_model.py, checked.  A scalar that fails is a finding: it belongs in special_scalars()."""
    S = M.special_scalars()
    rng = np.random.default_rng(2718)
    raw = rng.integers(0, 1 << 32, size=(100_000, 8), dtype=np.uint64).astype(object)
    rnd = [int(v) % R for v in sum(raw[:, j] << (32 * j) for j in range(8))]
    vals = S + rnd
    sp = M.splits(cm, vals, False)
    # the special scalars one by one through the model proper, with the trace's shape
    for v, split in zip(S, sp):
        events, u = M.single_chain(split)
        assert u == v and not M.exceptional(events), hex(v)
        assert [e[2] for e in events] == ([M.INTO_INF] + [M.PLAIN] * (len(events) - 1) if v else []), hex(v)
    # ... and everything through the same recurrence on arrays; what it reports is shown by the model proper
    bad = M.single_chains_have_no_exceptional_step(sp, vals)
    assert not bad, [(hex(vals[i]), M.exceptional(M.single_chain(sp[i])[0])) for i in bad[:5]]


def test_the_array_form_of_the_single_chain_sees_an_exceptional_step():
    """single_chains_have_no_exceptional_step does report a chain that meets one.  No split of 127-bit halves does
    under the real lambda, so the check runs over a toy eigenvalue: with lambda = 2 the halves a = 2, b = 1 reach
    u = 2 before the addend 2 (equal), and with the second sign negative u = 2 before -2 (opposite)."""
    for split, kind in (((2, 1, 1, 1), M.EQUAL), ((2, 1, 1, -1), M.OPPOSITE), ((3, 1, 1, 1), None)):
        events, u = M.single_chain(split, lam=2)
        assert [e[2] for e in M.exceptional(events)] == ([kind] if kind else [])
        assert M.single_chains_have_no_exceptional_step([split], [u], lam=2) == ([0] if kind else [])
        assert M.single_chains_have_no_exceptional_step([split], [u + 1], lam=2) == [0]     # a wrong end is reported too


# ------------------------------------------------------------------------- the committed tracker members ---
@pytest.fixture(scope="module")
def fixture_rows():
    return gen.load()


def test_the_fixture_has_every_required_class(fixture_rows):
    rows, tried, found = fixture_rows
    for cls in (1, 2, 6, 7):                                   # reachable with k = +-1 (or k = 0): must be there
        assert found[cls] == gen.PER_CLASS, cls
    for cls in gen.CLASSES:
        mine = [r for r in rows if r["cls"] == cls]
        assert len(mine) == found[cls] and len({r["seed"] for r in mine}) == len(mine)
        assert tried[cls] <= gen.BUDGET and (found[cls] == gen.PER_CLASS or tried[cls] == gen.BUDGET), cls
    assert os.path.getsize(gen.OUT) < 64 * 1024


def test_the_fixture_members_are_this_projects_proofs_and_take_their_branch(cm, oracle, fixture_rows):
    """Every member is regenerated byte for byte from (k, r, seed) by the project's prover, is accepted by the
    single call, and its trace over the HOST build of the split holds the recorded step and still belongs to
    its class; for k != 0 the challenge implied by s is the transcript's (tests/merlin_model.py)."""
    rows, _, _ = fixture_rows
    maker = gen.Maker(cm, oracle)
    for row in rows:
        k, r, seed = row["k"], row["r"], row["seed"]
        assert maker.member(k, r, seed) == row["member"], (row["cls"], seed)
        assert cm.whisk_is_valid_tracker_proof(*row["member"]) is True
        events = gen.trace_of(cm, oracle, row["member"], k, r, seed, on_device=False)
        assert (row["bit"], row["site"], row["step"]) in events, (row["cls"], seed)
        assert gen.classes_of(events, k, r).get(row["cls"]) == (row["bit"], row["site"], row["step"])
        if k:
            s, c, b = gen.member_scalars(oracle, row["member"], k, seed)
            assert c == gen.transcript_challenge(*row["member"], oracle.compress(oracle.G1))


def test_the_search_finds_the_committed_members_again(cm, oracle, fixture_rows):
    """The head of the generator's search (as many candidates as the slowest found class needed) gives the
    committed rows of every found class: the file is what its script writes."""
    rows, tried, found = fixture_rows
    budget = max(tried[c] for c in gen.CLASSES if found[c] == gen.PER_CLASS)
    assert budget <= 2_000
    again, tried2, found2 = gen.search(cm, oracle, budget=budget)
    as_rows = [(r["cls"], r["k"], r["r"], r["seed"], r["member"], r["bit"], r["site"], r["step"]) for r in rows]
    assert again == as_rows
    for c in gen.CLASSES:
        if found[c] == gen.PER_CLASS:
            assert (tried2[c], found2[c]) == (tried[c], found[c])
