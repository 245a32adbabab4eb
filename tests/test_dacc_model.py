"""The big-integer model of the device accumulator (tests/dacc_model.py) made trustworthy before it
judges a kernel (tests/test_dacc_direct_gpu.py): the generator's coverage claims proved by
assertion, algebraic identities a transliteration of the kernel would not satisfy by construction,
and the model against an independent C++ implementation -- the host stand-in of
tests/hostbuild/stub_backend.cpp (alg::Scalar, textbook double-and-add) driven through the public
entry points by `host_flow dacc` under AddressSanitizer + UBSan -- and against the C oracle's MSM.
No GPU."""
import os

import numpy as np
import pytest

import dacc_model as M
from dacc_model import CONST, EXPLICIT, FOLD, FOLD_POW, R, SET_CRS, SET_INST, Check, Seg
from test_host_sanitize import _run, harness  # noqa: F401  (the shared sanitizer build)

STAND_IN_MAX = 700      # scalar multiplications per case the naive stand-in is given (cases beyond: model and GPU only)


@pytest.fixture(scope="module")
def cases():
    return {f: M.family(f) for f in M.FAMILIES}


@pytest.fixture(scope="module")
def base_pts(cm):
    return cm.Rand(2024).get_g1_affines(257)


# ------------------------------------------------------------------- what the generator claims ---
def test_every_generated_case_is_a_valid_description(cases):
    for fam, cs in cases.items():
        assert cs, fam
        for c in cs:
            assert M.validate(c.checks, len(c.pool), c.n_crs, c.n_inst, c.n_extra), c.name
            assert len(c.extra_scalars) == c.n_extra and all(0 <= v < R for v in c.pool + list(c.extra_scalars)), c.name
            assert c.inf_inst < c.n_inst and c.inf_extra < c.n_extra, c.name
    assert len({c.name for cs in cases.values() for c in cs}) == sum(len(cs) for cs in cases.values())
    assert M.family("random") == M.family("random")                      # the same on every call
    assert len(cases["random"]) >= 200
    assert all(c.n_res <= 600 and len(c.checks) <= 12 for c in cases["random"])
    assert {k.kind for c in cases["random"] for k in c.checks} == {EXPLICIT, CONST, FOLD, FOLD_POW}
    assert {len(k.segs) for c in cases["random"] for k in c.checks} == set(range(7))
    wide = cases["random_wide"]
    assert all(c.n_res <= 600 and len(c.checks) <= 12 for c in wide) and max(c.n_res for c in wide) > 512
    assert sum(c.n_res > 256 for c in wide) >= len(wide) // 2                 # most span several blocks of the front
    assert {k.kind for c in wide for k in c.checks} == {EXPLICIT, CONST, FOLD, FOLD_POW}


def test_validate_refuses_what_the_header_refuses():
    good = Check(FOLD_POW, 8, 3, 2, 0, 1, 2, 5, 6, 2, (Seg(SET_CRS, 0, 8, 2),))
    assert M.validate([good], 8, 8, 4, 0)
    bad = [good._replace(kind=4), good._replace(m=32), good._replace(n_struct=9), good._replace(weight_off=8),
           good._replace(alpha_off=8), good._replace(gammas_off=6), good._replace(q_off=8), good._replace(tail_off=7),
           good._replace(n_tail=3), good._replace(kind=EXPLICIT), good._replace(segs=(Seg(2, 0, 8, 2),)),
           good._replace(segs=(Seg(SET_CRS, 1, 8, 2),)), good._replace(segs=(Seg(SET_INST, 0, 5, 0),)),
           good._replace(segs=(Seg(SET_CRS, 0, 8, 3),)), good._replace(segs=(Seg(SET_CRS, 0, 1, 0),) * 7),
           good._replace(kind=CONST, n_struct=(1 << 31) + 1), good._replace(kind=CONST, n_struct=(1 << 32) - 2)]
    for k in bad:
        assert not M.validate([k], 8, 8, 4, 0), k
    assert not M.validate([], 0, 0, 0, M.MAX_EXTRA + 1) and M.validate([], 0, 0, 0, M.MAX_EXTRA)
    # ignored fields are not checked: m and gammas_off of CONST, q_off of everything but FOLD_POW
    assert M.validate([good._replace(kind=CONST, m=31, gammas_off=1 << 30, q_off=1 << 30)], 8, 8, 4, 0)


def test_routes_family_lands_on_both_sides_of_every_border(cases):
    taken = {}
    for c in cases["routes"]:
        taken.setdefault(M.path(c.n_total, len(c.pool), len(c.checks)), []).append(c)
    assert set(taken) == {"front_lds", "front_global", "split_lds", "split_global"}
    for staged, walked, n, budget in (("front_lds", "front_global", M.FUSED_MAX, M.FRONT_BUDGET),
                                      ("split_lds", "split_global", M.FUSED_MAX + 1, M.SPLIT_BUDGET)):
        (a,), (b,) = taken[staged], taken[walked]
        assert a.n_total == b.n_total == n                                 # the 16,384 / 16,385 border, both sides
        assert len(b.pool) == len(a.pool) + 1 and len(a.checks) == len(b.checks)  # the pool border, both sides
        need = len(a.pool) * 32 + (len(a.checks) * 140 + 15) // 16 * 16 + 16
        assert need <= budget < need + 32
        # the pool's last element is read by a slot: a staging loop that stops short is seen
        for c in (a, b):
            assert any(k.tail_off + k.n_tail == len(c.pool) and any(s.vec_first + s.len == k.n_struct + k.n_tail for s in k.segs)
                       for k in c.checks), c.name
    assert M.path(0, 0, 0) == "none"
    # the other families reach the degenerate ends of the routing as well
    tot = {M.path(c.n_total, len(c.pool), len(c.checks)) for c in cases["totals"]}
    assert {"none", "front_lds", "split_lds"} <= tot
    assert {c.n_total for c in cases["totals"]} >= {0, 1, 3, M.FUSED_MAX, M.FUSED_MAX + 1}
    assert {c.n_res for c in cases["totals"]} >= {1, 255, 256, 257, 511, 513}
    assert M.MAX_EXTRA in {c.n_extra for c in cases["totals"]}


def test_qpow_family_reaches_the_exponents_it_claims(cases):
    es = set()
    for c in cases["qpow"]:
        es |= M.exponents(c.checks)
    assert set(range(1, 18)) <= es
    assert {1 << k for k in range(0, 32)} <= es                           # 2^31: i = 2^31 - 1, every squaring of the loop
    assert {(1 << k) - 1 for k in range(1, 32)} <= es                     # all ones: a multiply after every squaring
    caps = {k.q_cap for c in cases["qpow"] for k in c.checks}
    assert {0, 1, 2, 3, 4, 7, 8, 19, 20, (1 << 31) - 1, (1 << 32) - 1} <= caps
    # a cap that bites inside a segment, and one that never does
    assert any(k.q_cap < s.vec_first + s.len - 1 for c in cases["qpow"] for k in c.checks for s in k.segs)
    # the kinds family: every kind at every size, m = 0, m beyond log2(n_struct), m = 31, products of 31 gammas
    seen = {(k.kind, k.n_struct + (k.n_tail if k.kind == EXPLICIT else 0)) for c in cases["kinds"] for k in c.checks}
    assert seen >= {(kind, n) for kind in range(4) for n in (1, 2, 3, 8, 13, 256, 1000)}
    ms = {(k.kind, k.m) for c in cases["kinds"] for k in c.checks}
    assert ms >= {(FOLD, 0), (FOLD, 31), (FOLD_POW, 0), (FOLD_POW, 31), (FOLD, 13), (FOLD_POW, 13)}
    assert any(k.n_struct == 1 << 31 and s.vec_first + s.len == 1 << 31 for c in cases["kinds"] for k in c.checks for s in k.segs)


def test_special_family_puts_every_constant_in_every_role_of_every_kind(cases):
    tags = set()
    for c in cases["special"]:
        tags |= c.tags
    roles = {EXPLICIT: ("alpha", "tail"), CONST: ("weight", "alpha", "tail"), FOLD: ("weight", "alpha", "tail", "gamma"),
             FOLD_POW: ("weight", "alpha", "tail", "gamma", "q")}
    assert tags == {(kind, role, v) for kind, rs in roles.items() for role in rs for v in M.SPECIALS}
    for c in cases["special"]:                       # the tag is true: the value sits where the tag says
        for kind, role, v in c.tags:
            k, val = c.checks[0], M.SPECIALS[v]
            where = {"alpha": [c.pool[k.alpha_off]], "weight": [c.pool[k.weight_off]], "q": [c.pool[k.q_off]],
                     "gamma": c.pool[k.gammas_off:k.gammas_off + k.m], "tail": c.pool[k.tail_off:k.tail_off + k.n_tail]}[role]
            assert k.kind == kind and val in where and val in c.extra_scalars, c.name
    assert any(c.inf_inst >= 0 for cs in cases.values() for c in cs) and any(c.inf_extra >= 0 for cs in cases.values() for c in cs)
    # tails / overlap: what their names say
    spans = {(s.vec_first + s.len <= k.n_struct, s.vec_first >= k.n_struct) for c in cases["tails"] for k in c.checks
             for s in k.segs if k.n_struct and k.n_tail}
    assert spans == {(True, False), (False, True), (False, False)}        # structured, tail, straddling
    assert any(len(k.segs) == 6 for c in cases["overlap"] for k in c.checks) and any(len(c.checks) == 8 for c in cases["overlap"])
    assert any(c.n_crs % 256 and {s.set for k in c.checks for s in k.segs} == {SET_CRS, SET_INST} for c in cases["overlap"])


# ------------------------------------------------------------------------------- identities ---
def _fold_check(kind, n_struct, m, q_cap=0, n_tail=0):
    """A check over a pool laid out as weight | alpha | gammas | q | tail."""
    return Check(kind, n_struct, m, q_cap, 0, 1, 2, 2 + m, 3 + m, n_tail, (Seg(SET_CRS, 0, n_struct + n_tail, 0),))


def _pool(rng, m, n_tail=0):
    return [M._fr(rng) for _ in range(3 + m + n_tail)]


def test_the_sum_of_a_fold_vector_is_the_product_of_one_plus_gamma():
    rng = np.random.default_rng(1)
    for m in range(0, 11):
        pool = _pool(rng, m)
        want = pool[0]
        for g in pool[2:2 + m]:
            want = want * (1 + g) % R
        assert sum(M.vector(_fold_check(FOLD, 1 << m, m), pool)) % R == want, m


def test_fold_vector_equals_the_references_constructions():
    """innerproductargument.go:225-234 (for every i, the bits of i pick gamma[m-j-1]) and the halving
    recursion the prover folds by (x = x_lo ++ gamma_first * x_lo); the powers of q as the running
    product of grandproductargument.go:234-242, which stops growing at the cap."""
    rng = np.random.default_rng(2)
    for m in range(0, 9):
        for n in sorted({1, (1 << m) // 2 + 1, (1 << m) - 1, 1 << m} - {0}):
            pool = _pool(rng, m)
            gam, w, q = pool[2:2 + m], pool[0], pool[2 + m]
            ref = []
            for i in range(n):
                s = 1
                for j in range(m):
                    if i & (1 << j):
                        s = s * gam[m - j - 1] % R
                ref.append(w * s % R)

            def halves(gs):
                if not gs:
                    return [w]
                lo = halves(gs[1:])
                return lo + [gs[0] * x % R for x in lo]
            assert M.vector(_fold_check(FOLD, n, m), pool) == ref == halves(gam)[:n], (m, n)
            assert [M.element(_fold_check(FOLD, n, m), pool, i) for i in range(n)] == ref
            for cap in (0, 1, n // 2, n - 1, n, 1 << 32 - 1):
                run, pw = [], q
                for i in range(n):
                    run.append(ref[i] * pw % R)
                    if i < cap:
                        pw = pw * q % R
                ck = _fold_check(FOLD_POW, n, m, cap)
                assert M.vector(ck, pool) == run == [M.element(ck, pool, i) for i in range(n)], (m, n, cap)


def test_fold_pow_with_q_one_is_fold_and_the_tail_is_alpha_times_the_tail():
    rng = np.random.default_rng(3)
    for m, n, cap in ((0, 1, 0), (3, 7, 2), (5, 32, 40), (6, 33, 1 << 31)):
        pool = _pool(rng, m, 4)
        pool[2 + m] = 1
        a, b = M.vector(_fold_check(FOLD_POW, n, m, cap, 4), pool), M.vector(_fold_check(FOLD, n, m, cap, 4), pool)
        assert a == b and a[n:] == [pool[1] * t % R for t in pool[3 + m:]]
        assert M.vector(_fold_check(CONST, n, m, cap, 4), pool) == [pool[0]] * n + a[n:]
        assert M.vector(_fold_check(EXPLICIT, 0, m, cap, 4), pool) == a[n:]


def test_element_agrees_with_vector_on_every_small_generated_check(cases):
    for cs in cases.values():
        for c in cs:
            for k in c.checks:
                if k.n_struct + k.n_tail <= 2048:
                    assert M.vector(k, c.pool) == [M.element(k, c.pool, i) for i in range(k.n_struct + k.n_tail)], c.name


def test_slots_do_not_depend_on_how_the_checks_are_split_or_ordered(cases):
    rng = np.random.default_rng(4)
    for c in cases["random"] + cases["overlap"] + cases["totals"][:8]:
        want = M.slots(c.checks, c.pool, c.n_crs, c.n_inst)
        split = []
        for k in c.checks:
            h = len(k.segs) // 2
            split += [k._replace(segs=k.segs[:h]), k._replace(segs=k.segs[h:])]
        assert M.slots(split, c.pool, c.n_crs, c.n_inst) == want, c.name
        order = rng.permutation(len(split))
        assert M.slots([split[i] for i in order], c.pool, c.n_crs, c.n_inst) == want, c.name
    # and against a per-slot restatement of the header's sentence on one family
    for c in cases["overlap"]:
        want = [0] * c.n_res
        for k in c.checks:
            x = M.vector(k, c.pool)
            for s in k.segs:
                for j in range(s.len):
                    want[(0 if s.set == SET_CRS else c.n_crs) + s.first + j] += x[s.vec_first + j]
        assert M.slots(c.checks, c.pool, c.n_crs, c.n_inst) == [v % R for v in want]


def test_packing_is_the_abi_layout(oracle):
    k = Check(3, 8, 3, 2, 11, 12, 13, 14, 15, 2, (Seg(1, 4, 5, 6), Seg(0, 7, 8, 9)))
    w = M.pack_checks([k, k])
    assert w.shape == (2, 35) and w.dtype == np.uint32
    assert list(w[1][:19]) == [3, 8, 3, 2, 11, 12, 13, 14, 15, 2, 2, 1, 4, 5, 6, 0, 7, 8, 9] and not w[1][19:].any()
    vals = [0, 1, R - 1, 12345]
    assert M.unpack_fr(M.pack_fr(vals, oracle), oracle) == vals
    assert M.raw_ints(M.pack_fr([1], oracle)) == [oracle.R_FR]


# ------------------------------------------------------- the model against the C++ stand-in ---
@pytest.mark.parametrize("fam", M.FAMILIES)
def test_model_matches_the_host_stand_in_and_the_oracle_msm(harness, cases, base_pts, oracle, coracle, tmp_path, fam):  # noqa: F811
    """Every family through curdle_dacc_begin / curdle_dacc_run with export_scalars in the sanitizer
    build (the stand-in's restatement over alg::Scalar and its textbook MSM): exported scalars ==
    slots(), bit for bit and canonical; the sum == the C oracle's MSM of (bases, model scalars ++ loose
    scalars); up to four cases of a family with at most 12 pairs also == the Python oracle's textbook sum
    (a cross-check of the C oracle: it is the C oracle that judges every case).  The two-step form gives
    the same."""
    todo = [c for c in cases[fam] if M.stand_in_cost(c) <= STAND_IN_MAX]
    if fam == "random_wide":
        todo = todo[:5]                                   # ~4 ms per non-zero slot here; the GPU file runs all of them
    assert todo and (len(todo) == len(cases[fam]) or fam in ("totals", "routes", "kinds", "random_wide")), fam
    if fam == "routes":
        assert len(todo) == len(cases[fam])               # all four builds' cases fit the stand-in
    path = os.path.join(tmp_path, "cases.bin")
    outs = []
    for two_step in ((False, True) if fam in ("totals", "overlap") else (False,)):
        with open(path, "wb") as f:
            f.write(M.pack_case_file(todo, base_pts, oracle, two_step))
        out = _run(harness, "dacc", path)
        assert f"dacc: {len(todo)} cases" in out
        outs.append(M.parse_case_output(out))
    assert all(o == outs[0] for o in outs)
    python_sums = 0
    for c, (rc, exported, total) in zip(todo, outs[0]):
        assert rc == 0, c.name
        want = M.slots(c.checks, c.pool, c.n_crs, c.n_inst)
        assert all(v < R for v in exported), c.name
        assert [v * oracle.R_FR_INV % R for v in exported] == want, c.name
        crs, inst, loose = M.case_points(c, base_pts)
        pts = np.concatenate([crs, inst, loose])
        sc = want + list(c.extra_scalars)
        exp = coracle.msm_pippenger(pts, M.pack_fr(sc, oracle), threads=4) if len(pts) else None
        if exp is None:
            exp = coracle.msm_pippenger(np.zeros((1, 12), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64))
        assert total == [int(v) for v in exp], c.name
        if c.n_total <= 12 and python_sums < 4:
            python_sums += 1
            acc = oracle.INF
            for p, s in zip(pts, sc):
                if p.any():
                    acc = oracle.add(acc, oracle.scalar_mul(s, oracle.affine_from_mont_limbs([int(v) for v in p])))
            assert total == [int(v) for v in coracle.jac_normalise(np.array(oracle.jac_to_mont_limbs(acc), dtype=np.uint64))], c.name


def test_the_stand_in_refuses_an_explicit_check_with_a_structured_part(harness, base_pts, oracle, tmp_path):  # noqa: F811
    """The header: EXPLICIT is x_i = tail[i], n_struct must be 0 (CURDLE_EINVAL = -1 otherwise)."""
    b = M._Builder(np.random.default_rng(9))
    b.check(CONST, 4, tail=[5, 6], segs=[(SET_CRS, 0, 6, 0)])
    ok = b.case(6, 0, 0, "", "const")
    bad = ok._replace(checks=[ok.checks[0]._replace(kind=EXPLICIT)])
    assert not M.validate(bad.checks, len(bad.pool), 6, 0, 0)
    path = os.path.join(tmp_path, "explicit.bin")
    with open(path, "wb") as f:
        f.write(M.pack_case_file([ok, bad], base_pts, oracle))
    res = M.parse_case_output(_run(harness, "dacc", path))
    assert [r[0] for r in res] == [0, -1]
