"""tests/golden/affine_check_points.npz cannot drift from its generator: a sample of every family is
rebuilt from the oracle and the definitions and compared with the committed words and statuses, the
families have at least the stated sizes and statuses, and the serialisation is reproducible."""
import importlib.util
import os
import sys
from collections import Counter

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "affine_check_points.npz")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_affine_check_points", os.path.join(GOLDEN, "gen_affine_check_points.py"))
    mod = importlib.util.module_from_spec(spec)
    path = list(sys.path)
    try:
        spec.loader.exec_module(mod)           # imports the decoder fixture's generator from its own directory
    finally:
        sys.path[:] = path
    return mod


@pytest.fixture(scope="module")
def committed():
    return np.load(FIXTURE)


def test_families_and_statuses_of_the_committed_file(gen, committed):
    fam = [f.decode() for f in committed["family"]]
    count = Counter(fam)
    assert list(dict.fromkeys(fam)) == list(gen.FAMILIES)          # every family present, in the generator's order
    assert all(count[f] >= gen.MINIMUM[f] for f in gen.FAMILIES), count
    n = len(fam)
    assert committed["points"].shape == (n, 12) and committed["points"].dtype == np.uint64
    sub, nosub = committed["status_subgroup"], committed["status_no_subgroup"]
    assert (nosub == np.where(sub == gen.NOT_IN_SUBGROUP, gen.OK, sub)).all()
    by = lambda f, st=sub: {int(s) for s, g in zip(st, fam) if g == f}
    assert by("from_decoder") == {gen.OK, gen.NOT_IN_SUBGROUP} and by("from_decoder", nosub) == {gen.OK}
    assert by("other_curve") == by("mixed") == {gen.NOT_ON_CURVE}
    assert by("other_curve", nosub) == by("mixed", nosub) == {gen.NOT_ON_CURVE}   # with and without the subgroup test
    assert by("range") == {gen.BAD_ENCODING} and by("infinity") == {gen.INFINITY}
    assert os.path.getsize(FIXTURE) < 100 * 1024


def test_from_decoder_is_every_decoder_record_that_has_a_point(gen, committed, oracle):
    z = np.load(os.path.join(GOLDEN, "decode_edge_records.npz"))
    rows = np.nonzero(z["status_no_subgroup"] == gen.OK)[0]
    mine = np.nonzero(committed["family"] == b"from_decoder")[0]
    assert len(rows) == len(mine)
    assert (committed["status_subgroup"][mine] == z["status_subgroup"][rows]).all()
    assert {f.decode() for f in z["family"][rows]} == {"g1", "torsion", "torsion_plus_g1", "composite", "cleared", "x_on_curve",
                                                      "sign_edge"}
    for i, j in list(zip(rows, mine))[::7]:
        b = z["points"][i].tobytes()
        x, y = int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big")
        assert committed["points"][j].tolist() == list(oracle.fp_to_mont_limbs(x)) + list(oracle.fp_to_mont_limbs(y))


def test_the_other_curve_family_holds_what_the_check_exists_for(gen, committed, oracle):
    rows = np.nonzero(committed["family"] == b"other_curve")[0]
    seen, bs = set(), Counter()
    for i in rows:
        w = committed["points"][i].tolist()
        x, y = oracle.fp_from_mont_limbs(w[:6]), oracle.fp_from_mont_limbs(w[6:])
        b = (y * y - x * x * x) % oracle.P
        assert b in gen.OTHER_B and b != 4
        bs[b] += 1
        seen.add((x, y))
    assert all(bs[b] == 16 for b in gen.OTHER_B), bs
    assert {(0, 1), (0, oracle.P - 1), (0, 3), (0, oracle.P - 3)} <= seen


@pytest.mark.parametrize("family", ["from_decoder", "other_curve", "mixed", "range", "infinity"])
def test_a_sample_of_every_family_regenerates(gen, committed, family):
    """The first entries of the family, rebuilt with every self-check of the generator (the definitional
    statuses, what each family was built to be) == the committed ones."""
    take = {"from_decoder": 24, "other_curve": 20, "mixed": 12, "range": 18, "infinity": 1}[family]
    rows = np.nonzero(committed["family"] == family.encode())[0][:take]
    got = gen.entries(family, take)
    assert len(got) == take == len(rows)
    for i, (w, st_sub, st_nosub) in zip(rows, got):
        assert committed["points"][i].tolist() == list(w)
        assert (int(committed["status_subgroup"][i]), int(committed["status_no_subgroup"][i])) == (st_sub, st_nosub)


def test_serialisation_is_reproducible(gen, committed):
    arrs = {k: committed[k] for k in ("points", "status_subgroup", "status_no_subgroup", "family")}
    with open(FIXTURE, "rb") as f:
        assert gen.dec.npz_bytes(arrs) == f.read()
