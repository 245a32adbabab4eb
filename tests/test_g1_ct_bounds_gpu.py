"""The constant-time G1 layer (csrc/g1_walk_ct.h, g1_add_ct.h, g1_exit_ct.h, invert28.h, madd_select of fbase_walk_ct.h)
on raw limbs, word for word against the limb-exact model of tests/g1_ct_model.py.  Selftest operation 16 calls the
production function of each header on the words a test writes; the case sets are those of tests/g1_ct_cases.py, which
tests/test_g1_ct_model.py checks against plain integers and the group law, arm by arm, without a GPU.  Integer
arithmetic: no tolerance, nothing filtered.  One launch per family; each boundary family runs whole."""
import numpy as np
import pytest

import fp28_model as m
import g1_ct_cases as c
import g1_ct_model as g

pytestmark = pytest.mark.gpu
P = m.P


def device(gpu, inp):
    return gpu.selftest_op(16, inp.astype(np.uint32), True).astype(np.uint64)


def same_words(dev, model, what):
    bad = np.flatnonzero((dev != model).any(axis=1))
    assert not len(bad), f"{what}: {len(bad)} of {len(dev)} elements differ, first {bad[0]}: {dev[bad[0]]} != {model[bad[0]]}"


def run(gpu, fams, name):
    out = {}
    for fam, v in fams.items():
        inp = v[0] if isinstance(v, tuple) else v
        out[fam] = device(gpu, inp)
        same_words(out[fam], c.model_out(inp), f"{name} {fam}")
    return out


@pytest.mark.parametrize("name", ["zero_mask", "finite_mask"])
def test_masks_on_every_single_bit(gpu, name):
    """All zero, each single bit of each word (14 x 32, 24 x 32), all ones, bits set only behind the operand, and 2^14 random."""
    out = run(gpu, c.mask_families(name), name)
    assert len(set(out["one_hot"][:, 56])) == 1 and out["one_hot"][0, 56] != out["all_zero"][0, 56]


def test_equal_mod_p_on_every_representative_pair_and_one_limb_differences(gpu):
    """Every representative pair of a < 2p, b < 10p for the residues 0, 1, p - 1 and random ones, the same off by one, reduced
    differences off 0 or p in exactly one limb (each of the 14), the four corners, 2^14 random pairs."""
    out = run(gpu, c.equal_families(), "equal_mod_p")
    assert (out["representatives"][:, 56] == 0xFFFFFFFF).all() and (out["off_by_one"][:, 56] == 0).all()


@pytest.mark.parametrize("name", list(c.EXIT_TABLE))
def test_the_masked_canonical_step_at_its_boundary(gpu, name):
    """to_gnark_ct with each constant on products t = 0, 1, p - 1, p (from p and from 9p), p + 1 and the largest any input
    below 10p gives, the field tests' edge list below 2p and 10p, 256 inputs built to subtract and 2^14 random ones;
    three ways: the model's words, and the words selftest operation 13 returns for the non-constant-time twin.
    The largest t / p reached, which is the largest any input below 10p can give: 1.003299 (kToExt), 1.001838
    (kToExtX16), 1.000188 (kToExtY64)."""
    fams = c.exit_families(name)
    out = run(gpu, fams, name)
    table = c.EXIT_TABLE[name]
    sel13 = 21 if table == "kToExt" else 22 + c.twin_role(table)      # to_gnark, or to_gnark_msm with the role of this table
    for fam, inp in fams.items():
        twin = np.zeros((len(inp), 60), dtype=np.uint32)
        twin[:, 0] = sel13
        twin[:, 4:18] = inp[:, 4:18]
        same_words(out[fam][:, :14], gpu.selftest_op(13, twin, True)[:, :14].astype(np.uint64), f"{name} {fam} against the twin")


def test_invert_words_and_products(gpu):
    """0, one, p - 1, p, p + 1, 2p - 1 and 2^10 random values below 2p: the model's words, and input times output is one
    (zero for the two representatives of zero)."""
    fams = c.invert_families()
    out = run(gpu, fams, "invert")
    for fam, inp in fams.items():
        for x, y in zip(m.value(inp[:, 4:18]), m.value(out[fam][:, :14])):
            assert m.from_mont(x) * m.from_mont(y) % P == (1 if x % P else 0)


def test_affine_words_ct_at_the_stored_bounds(gpu):
    """Finite points at x in [9p, 10p), y in [5p, 6p) and in [9p, 10p), zz, zzz in [p, 2p); the same below p; the all-zero
    record; four ones; records whose x, y or both take the subtracting arm of the canonical step."""
    run(gpu, c.affine_families(), "affine_words_ct")


@pytest.mark.parametrize("name", ["madd_bit", "madd_select"])
def test_the_step_addition_under_all_four_masks(gpu, name):
    """Generic operands, the accumulator at its stored bounds with the affine operand in [p, 2p), the nonsense sums P = acc
    and P = -acc under a scaling, and four ones doubled 0, 1, 2 and 254 times: every (bit, started) combination."""
    run(gpu, c.madd_families(name), name)


def test_add_ct_in_all_five_arms(gpu):
    """The five arms, the four infinity combinations, the same point and a point and its negative under independent
    scalings, operands at x, y in [9p, 10p) and zz, zzz in [p, 2p)."""
    out = run(gpu, c.add_families(), "add_ct")
    assert (out["opposite"][:, :56] == 0).all() and (out["opposite_below_p"][:, :56] == 0).all()


def test_a_fold_of_nine_terms_level_by_level(gpu):
    """k_g1_sum_ct's order over nine terms, each level's device output the next level's input: every level is the model's,
    so an output of add_ct is a legal input of it."""
    terms, _ = c.fold_terms()

    def on_device(a, b):
        out = device(gpu, c.block("add_ct", a[0].shape[0], A=a, B=b))
        return tuple(out[:, 14 * j:14 * (j + 1)] for j in range(4))

    dev = c.fold_levels(terms, on_device)
    mdl = c.fold_levels(terms, lambda a, b: g.add_ct(a, b)[0])
    assert len(dev) == len(mdl) == 4
    for lv, (d, e) in enumerate(zip(dev, mdl)):
        same_words(np.concatenate(d, axis=1), np.concatenate(e, axis=1), f"fold level {lv + 1}")


def test_walk_ct_at_every_step_count(gpu):
    """1, 2, 9, 64 and 255 steps on 0, 1, 2, 3, 2^(steps-1), 2^steps - 1; at 255 also r - 1, r - 2, (r -+ 1) / 2 and random
    scalars; scalars with a bit at or above `steps` (the `over` word); affine operands in [p, 2p)."""
    inp, info, n_plain = c.walk_families()
    out = device(gpu, inp)
    same_words(out, c.model_out(inp), "walk_ct")
    assert (out[:n_plain, 57] == 0).all() and (out[n_plain:, 57] == 1).all()
