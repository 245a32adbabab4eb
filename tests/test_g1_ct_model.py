"""The limb-exact model of the constant-time G1 layer (tests/g1_ct_model.py) and the case sets of selftest operation 16
(tests/g1_ct_cases.py), without a GPU: the model against arithmetic it does not share (plain Python integers and the
group operations of oracle/py), every family present and accepted by the model's contracts, every arm and boundary
reached by count, and every deliberately wrong variant of the model caught by the cases the GPU tests run.

Unreachable inside the stated bounds, asserted by the model on every call instead of tested:
  equal_mod_p's `e == 0` leg: a < 2p and b < 10p make the difference a - b + 16p at least 6p, never the integer 0, so the
  product by one is p, never 0, for congruent operands.
Equivalent variant (listed, not detected): "the canonical step masks the top limb of the difference".  The difference is
taken only when no borrow leaves the top limb, and then d[13] = t[13] - p[13] - borrow lies in [0, 2^28): the mask
changes no word that is ever selected.
"""
import functools
import json
import os

import numpy as np
import pytest

import bls12381_ref as oracle
import fp28_model as m
import g1_ct_cases as c
import g1_ct_model as g

P = m.P
EQUIVALENT = {"canonical_masks_top_limb"}


@functools.lru_cache(maxsize=None)
def families(name):
    return {"zero_mask": lambda: c.mask_families("zero_mask"), "finite_mask": lambda: c.mask_families("finite_mask"),
            "equal_mod_p": c.equal_families, "to_gnark_ct": lambda: c.exit_families("to_gnark_ct"),
            "to_gnark_ct_x16": lambda: c.exit_families("to_gnark_ct_x16"), "to_gnark_ct_y64": lambda: c.exit_families("to_gnark_ct_y64"),
            "invert": c.invert_families, "affine_words_ct": c.affine_families, "madd_bit": lambda: c.madd_families("madd_bit"),
            "madd_select": lambda: c.madd_families("madd_select"), "add_ct": c.add_families}[name]()


def _inp(v):
    return v[0] if isinstance(v, tuple) else v


@functools.lru_cache(maxsize=None)
def expected(name):
    """{family: (model words, the COUNTS the family added)}: computed once."""
    out = {}
    for fam, v in families(name).items():
        assert _inp(v).shape[0] > 0, (name, fam)
        g.COUNTS.clear()
        out[fam] = (c.model_out(_inp(v)), dict(g.COUNTS))           # a contract violation raises here
    return out


def counts(name):
    tot = {}
    for _, cnt in expected(name).values():
        for k, v in cnt.items():
            tot[k] = tot.get(k, 0) + v
    return tot


def _pt(words):
    return tuple(words[:, 14 * j:14 * (j + 1)] for j in range(4))


# --------------------------------------------------------------------------------------- masks, equality ---
def test_masks_read_every_bit_of_their_operand_and_nothing_else():
    for name, width in (("zero_mask", 14), ("finite_mask", 24)):
        exp = expected(name)
        assert set(exp) == {"all_zero", "one_hot", "all_ones", "behind_the_operand", "random"}
        nonzero = 0 if name == "zero_mask" else 0xFFFFFFFF
        assert exp["one_hot"][0].shape[0] == width * 32
        assert (exp["one_hot"][0][:, 56] == nonzero).all() and (exp["all_ones"][0][:, 56] == nonzero).all()
        assert (exp["all_zero"][0][:, 56] == (0xFFFFFFFF ^ nonzero)).all()
        assert (exp["behind_the_operand"][0][:, 56] == (0xFFFFFFFF ^ nonzero)).all()
        inp = families(name)["random"]
        plain = (inp[:, 4:4 + width] != 0).any(axis=1)
        assert ((exp["random"][0][:, 56] == nonzero) == plain).all() and 0 < plain.sum() < len(plain)


def test_equal_mod_p_against_integers_and_its_dead_leg():
    exp = expected("equal_mod_p")
    assert set(exp) == {"representatives", "off_by_one", "one_limb", "corners", "random"}
    for fam, inp in families("equal_mod_p").items():
        a, b = m.value(inp[:, 4:18]), m.value(inp[:, 18:32])
        want = [0xFFFFFFFF if (x - y) % P == 0 else 0 for x, y in zip(a, b)]
        assert list(exp[fam][0][:, 56]) == want, fam
        assert all(x < 2 * P and y < 10 * P and x - y + 16 * P >= 6 * P for x, y in zip(a, b))
    assert (exp["representatives"][0][:, 56] == 0xFFFFFFFF).all() and (exp["off_by_one"][0][:, 56] == 0).all()
    assert (exp["one_limb"][0][:, 56] == 0).all()
    tot = counts("equal_mod_p")
    assert tot["equal:e==p"] >= 160 + 8000 and tot["equal:neither"] > 8000
    assert tot["equal:e==0"] == 0                       # unreachable: the model raises if it ever happens
    with pytest.raises(g.ContractError):                # and the unreachability rests on the contract: out of it, no promise
        g.equal_mod_p(m.arr([2 * P]), m.arr([0]))


# ----------------------------------------------------------------------------------------------- the exit ---
@pytest.mark.parametrize("name", list(c.EXIT_TABLE))
def test_to_gnark_ct_is_the_canonical_product_and_both_arms_are_reached(name):
    table = c.EXIT_TABLE[name]
    const = m.value1(m._T[table])
    exp = expected(name)
    assert set(exp) == {"targets", "edges", "subtracting", "random"}
    for fam, inp in families(name).items():
        a = m.value(inp[:, 4:18])
        words = exp[fam][0][:, :12]
        got = [sum(int(x) << (32 * j) for j, x in enumerate(row)) for row in words]
        assert got == [v * const * m.RP_INV % P for v in a], fam               # canonical, as plain integers
        assert (words == m.to_gnark(inp[:, 4:18], table)[:, :12]).all(), fam   # and the non-constant-time twin's words
    # the products land where the builder aimed them
    tg = c.exit_targets(table)
    t = dict(zip(tg, g.exit_t(m.arr(list(tg.values())), table)))
    assert [t[k] for k in ("t=0", "t=1", "t=p-1", "t=p", "t=p_from_9p", "t=p+1")] == [0, 1, P - 1, P, P, P + 1]
    assert P < t["t=max"] < 2 * P and all(v < 10 * P for v in tg.values())
    tau = c.exit_tau_max(table)
    assert t["t=max"] == P + tau                          # the largest product any input below 10p gives: one more has no input
    for j in range(10):
        a = (tau + 1) * m.RP % P * pow(const, -1, P) % P + j * P
        assert g.exit_t(m.arr([a]), table)[0] == tau + 1
    cnt = exp["subtracting"][1]
    assert cnt[f"exit:{table}:t>=p"] == 256 and cnt.get(f"exit:{table}:t<p", 0) == 0
    tot = counts(name)
    assert tot[f"exit:{table}:t<p"] > 16000 and tot[f"exit:{table}:t>=p"] >= 256 + 4
    assert c.twin_role(table) == {"kToExt": 2, "kToExtX16": 0, "kToExtY64": 1}[table]


def test_invert_against_integers():
    exp = expected("invert")
    for fam, inp in families("invert").items():
        d, inv = m.value(inp[:, 4:18]), m.value(exp[fam][0][:, :14])
        for x, y in zip(d, inv):
            assert y < 2 * P
            assert m.from_mont(x) * m.from_mont(y) % P == (1 if x % P else 0)
    d = m.value(families("invert")["edges"][:, 4:18])
    assert d == [0, m.value1(m.KONE), P - 1, P, P + 1, 2 * P - 1]
    assert m.value(exp["edges"][0][:2, :14]) == [0, m.value1(m.KONE)]     # 0 -> 0 as an integer; one -> one


def test_affine_words_ct_against_integers_and_its_subtracting_arms():
    exp = expected("affine_words_ct")
    assert set(exp) == {"x<10p,y<6p", "y<10p", "below_p", "all_zero", "four_ones", "subtracting"}
    for fam, (inp, info) in families("affine_words_ct").items():
        words = exp[fam][0]
        for i, pt in enumerate(info):
            if pt is None:
                assert (words[i] == 0).all()
                continue
            assert g.gnark_value(words[i:i + 1, :12])[0] == pt[0] and g.gnark_value(words[i:i + 1, 12:24])[0] == pt[1], (fam, i)
    cnt = exp["subtracting"][1]
    assert cnt["affine:x>=p"] >= 4 and cnt["affine:y>=p"] >= 4 and cnt["affine:both>=p"] >= 4
    assert cnt["exit:kToExt:t>=p"] == cnt["affine:x>=p"] + cnt["affine:y>=p"] + 2 * cnt["affine:both>=p"]


# ----------------------------------------------------------------------------------------- the additions ---
@pytest.mark.parametrize("name", ["madd_bit", "madd_select"])
def test_the_step_additions_against_the_group_law(name):
    exp = expected(name)
    assert set(exp) == {"generic", "at_the_bounds", "P=acc", "P=-acc"} | {f"ones_doubled_{t}" for t in (0, 1, 2, 254)}
    one = np.array(m.KONE, dtype=np.uint64)
    kept = 0
    for fam, (inp, info) in families(name).items():
        out = _pt(exp[fam][0])
        acc, x2, y2 = c._pt(inp, 4), inp[:, 60:74], inp[:, 74:88]
        bit, started = inp[:, 1] != 0, inp[:, 2] != 0
        aff = m.affine(out)
        for i, (a, b) in enumerate(info):
            if bit[i] and started[i]:
                if fam in ("generic", "at_the_bounds"):            # a kept sum of a walk: distinct points, not opposite
                    assert aff[i] == oracle.add(a, b), (fam, i)
                    kept += 1
            elif bit[i]:                                           # the first addition: the affine point as it came, zz = zzz = one
                assert (out[0][i] == x2[i]).all() and (out[1][i] == m.norm(y2[i:i + 1])[0]).all()
                if name == "madd_bit":
                    assert (out[2][i] == one).all() and (out[3][i] == one).all()
                else:                                              # madd_select: zz * one, the same residue
                    assert m.value1(out[2][i]) % P == m.value1(acc[2][i]) % P and m.value1(out[3][i]) % P == m.value1(acc[3][i]) % P
                if name == "madd_bit" or fam == "ones_doubled_0":   # (madd_select keeps zz, which is one before the first addition)
                    assert aff[i] == b, (fam, i)
            else:                                                  # bit 0: the accumulator stays
                assert (out[0][i] == acc[0][i]).all() and (out[1][i] == acc[1][i]).all()
                if name == "madd_bit":
                    assert (out[2][i] == acc[2][i]).all() and (out[3][i] == acc[3][i]).all()
                else:
                    assert m.value1(out[2][i]) % P == m.value1(acc[2][i]) % P and m.value1(out[3][i]) % P == m.value1(acc[3][i]) % P
        cnt = exp[fam][1]
        for b in (0, 1):
            for s in (0, 1):
                assert cnt[f"{name}:bit={b},started={s}"] == len(info) // 4, (fam, b, s)
    assert kept == 2 * 128
    if name == "madd_select":       # digit 0 multiplies zz by one: in [p, 2p) the representative does change, and the model mirrors it
        inp, _ = families(name)["at_the_bounds"]
        out = exp["at_the_bounds"][0]
        idle = inp[:, 1] == 0
        assert (out[idle][:, 28:56] != inp[idle][:, 4 + 28:4 + 56]).any()


def _arm_of(a, b):
    if a is None:
        return 1
    if b is None:
        return 2
    if a == b:
        return 3
    if a == oracle.neg(b):
        return 4
    return 5


def test_add_ct_against_the_group_law_arm_by_arm():
    exp = expected("add_ct")
    arms = {k: 0 for k in range(1, 6)}
    for fam, (inp, info) in families("add_ct").items():
        out = _pt(exp[fam][0])
        _, arm = g.add_ct(c._pt(inp, 4), c._pt(inp, 60))
        aff = m.affine(out)
        for i, (a, b) in enumerate(info):
            assert arm[i] == _arm_of(a, b), (fam, i)        # equal x with different y is the negative and nothing else
            assert aff[i] == oracle.add(a, b), (fam, i)
            arms[int(arm[i])] += 1
        if fam.startswith("opposite"):
            assert (exp[fam][0][:, :56] == 0).all()          # arm 4: 56 zero words
        if fam.startswith("same_point"):                     # arm 3 on different words: the operands are scaled independently
            assert (inp[:, 4:60] != inp[:, 60:116]).any(axis=1).all()
    assert arms == {1: 32 + 4 + 8, 2: 32, 3: 64, 4: 64, 5: 3 * 256}
    tot = counts("add_ct")
    assert all(tot[f"add_ct:arm{k}"] == arms[k] for k in arms)


def test_the_fold_of_nine_terms_feeds_outputs_back_in():
    terms, pts = c.fold_terms()
    g.COUNTS.clear()
    levels = c.fold_levels(terms, lambda a, b: g.add_ct(a, b)[0])       # every level's operands pass add_ct's contract
    want = list(pts)
    mcount = 9
    for lv in levels:
        h = (mcount + 1) // 2
        for i in range(mcount - h):
            want[i] = oracle.add(want[i], want[i + h])
        mcount = h
        assert m.affine(lv) == want[:h]
    assert len(levels) == 4 and m.affine(levels[-1]) == [oracle.scalar_mul(63, c.G1)]
    assert g.COUNTS["add_ct:arm3"] == 2 and g.COUNTS["add_ct:arm4"] == 1 and g.COUNTS["add_ct:arm1"] == 2


# ------------------------------------------------------------------------------------------------ the walk ---
@functools.lru_cache(maxsize=None)
def walk_expected():
    inp, info, n_plain = c.walk_families()
    return inp, info, n_plain, c.model_out(inp)


def test_walk_ct_against_scalar_multiplication_at_every_step_count():
    inp, info, n_plain, out = walk_expected()
    aff = m.affine(_pt(out))
    seen = set()
    for i, (k, steps, pt) in enumerate(info):
        low = k & ((1 << steps) - 1)
        assert out[i, 56] == (0xFFFFFFFF if low else 0), i
        assert out[i, 57] == (1 if k >> steps else 0), i
        assert (i < n_plain) == (k >> steps == 0)
        if low and pt is not None:
            assert aff[i] == oracle.scalar_mul(low, pt), i
        seen.add(steps)
    assert seen == {1, 2, 9, 64, 255} and len(info) == 256
    at_top = [i for i, (_, _, pt) in enumerate(info) if pt is None]
    assert len(at_top) == 12 and all(2 * P - 1 in (m.value1(inp[i, 4:18]), m.value1(inp[i, 18:32])) for i in at_top)
    ks255 = {k for k, s, _ in info if s == 255}
    assert {0, 1, 2, 3, 1 << 254, (1 << 255) - 1, c.R - 1, c.R - 2, (c.R - 1) // 2, (c.R + 1) // 2} <= ks255


def test_the_golden_exit_edges_take_the_subtracting_arm_in_the_model():
    """tests/golden/ct_exit_edges.json (tools/find_ct_exit_edges.py): every entry, re-checked."""
    doc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ct_exit_edges.json")))
    ent = doc["entries"]
    assert doc["searched"]["pairs"] == doc["searched"]["points_j"] * 3 >= 3 << 21
    assert doc["found"]["x"] > 0 and doc["found"]["y"] > 0 and {e["kind"] for e in ent} >= {"x", "y"}
    for k in (1, 2, 3):
        some = [e for e in ent if e["k"] == k]
        if not some:
            continue
        pts = [oracle.scalar_mul(e["j"], c.G1) for e in some]
        gx, gy, acc = g.mul_ct_exit(k, pts)
        assert m.affine(acc) == [oracle.scalar_mul(k * e["j"], c.G1) for e in some]
        for e, sx, sy in zip(some, gx, gy):
            assert e["kind"] == ("both" if sx and sy else "x" if sx else "y" if sy else None), e


def test_the_golden_fixed_base_scalars_take_the_subtracting_arm_in_the_model():
    """The `fbase` section of tests/golden/ct_exit_edges.json: every scalar walked again against the generator's table by the
    model of k_fbase_mul_ct (64 windows of madd_select over the words from_gnark_iso gives the multiples), its exits
    re-classified, and the 48 words the kernel stores checked against the group law."""
    doc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ct_exit_edges.json")))["fbase"]
    ent = doc["entries"]
    assert doc["searched"] == 1 << 17 and doc["found"]["x"] > 0 and doc["found"]["y"] > 0
    assert {e["kind"] for e in ent} >= {"x", "y"}
    ks = [int(e["k"], 16) for e in ent] + [0, 1, 16, c.R - 1]
    tab = g.fbase_window_table(oracle.add, c.G1)
    assert tab[2][:2] == [c.G1, oracle.add(c.G1, c.G1)] and tab[2][15] == oracle.scalar_mul(16, c.G1)
    g.COUNTS.clear()
    acc, started = g.fbase_walk_ct(g.scalar_words(ks), tab)
    sx, sy = g.exit_subtracts(acc[0], "kToExtX16"), g.exit_subtracts(acc[1], "kToExtY64")
    for e, a, b in zip(ent, sx, sy):
        assert e["kind"] == ("both" if a and b else "x" if a else "y" if b else None), e
    words = g.fbase_exit_words(acc, started)
    assert g.COUNTS["exit:kToExtX16:t>=p"] >= 4 and g.COUNTS["exit:kToExtY64:t>=p"] >= 2
    for i, k in enumerate(ks):
        if k == 0:
            assert (words[i] == 0).all() and started[i] == 0
            continue
        X, Y, ZZ, ZZZ = (g.gnark_value(words[i:i + 1, 12 * j:12 * j + 12])[0] for j in range(4))
        assert (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P) == oracle.scalar_mul(k, c.G1), hex(k)


# --------------------------------------------------------------------------------------- discrimination ---
def _changed(name, variant, fams=None):
    """Does the wrong variant change a word of the expected output of selector `name` (families `fams`, default all)?"""
    for fam, v in families(name).items():
        if fams is not None and fam not in fams:
            continue
        with g.wrong(variant):
            bad = c.model_out(_inp(v))           # an assertion of the model that fires here fails the test: only a changed word counts
        if (bad != expected(name)[fam][0]).any():
            return True
    return False


def test_every_wrong_variant_changes_an_expected_word():
    """A wrong kernel cannot be built into the suite, so the case sets are judged on wrong MODELS: each variant must
    change at least one word the GPU tests compare."""
    fast = {"targets", "edges", "subtracting"}
    caught = {}
    for v in ("canonical_never_subtracts", "canonical_subtracts_only_above_p", "canonical_masks_top_limb"):
        caught[v] = all(_changed(name, v, fast) for name in c.EXIT_TABLE)
    assert _changed("to_gnark_ct", "canonical_subtracts_only_above_p", {"targets"})
    assert _changed("affine_words_ct", "canonical_never_subtracts", {"subtracting"})
    caught["x16_exit_uses_kToExt"] = _changed("to_gnark_ct_x16", "x16_exit_uses_kToExt", fast)
    for j in range(m.N):
        caught[f"equal_drops_limb_{j}"] = _changed("equal_mod_p", f"equal_drops_limb_{j}", {"one_limb"})
    small = {"same_point", "opposite", "a_infinite", "both_infinite", "a_infinite_by_zz_alone"}
    caught["add_doubles_on_eq_x_alone"] = _changed("add_ct", "add_doubles_on_eq_x_alone", {"opposite", "opposite_below_p"})
    caught["add_takes_acc_when_a_inf"] = _changed("add_ct", "add_takes_acc_when_a_inf", small)
    caught["madd_bit_first_keeps_zz"] = _changed("madd_bit", "madd_bit_first_keeps_zz", {"at_the_bounds", "ones_doubled_1"})
    caught["invert_uses_t5_for_window_6"] = _changed("invert", "invert_uses_t5_for_window_6", {"edges"})
    inp, _, _, out = walk_expected()
    short = np.flatnonzero(inp[:, 1] <= 9)
    with g.wrong("walk_updates_started_first"):
        caught["walk_updates_started_first"] = bool((c.model_out(inp[short]) != out[short]).any())
    assert set(caught) == set(g.WRONG_VARIANTS)
    assert {v for v, ok in caught.items() if not ok} == EQUIVALENT
    assert not g.WRONG
