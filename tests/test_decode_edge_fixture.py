"""tests/golden/decode_edge_records.npz cannot drift from its generator: a sample of every family
is rebuilt from the oracle and the definitions and compared with the committed bytes, the families
have at least the stated sizes, and the serialisation is reproducible."""
import importlib.util
import os
from collections import Counter

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_decode_edge_records", os.path.join(GOLDEN, "gen_decode_edge_records.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def committed():
    return np.load(os.path.join(GOLDEN, "decode_edge_records.npz"))


def test_families_and_statuses_of_the_committed_file(gen, committed):
    fam = [f.decode() for f in committed["family"]]
    count = Counter(fam)
    assert list(dict.fromkeys(fam)) == list(gen.FAMILIES)          # every family present, in the generator's order
    assert all(count[f] >= gen.MINIMUM[f] for f in gen.FAMILIES), count
    n = len(fam)
    assert committed["records"].shape == (n, 48) and committed["points"].shape == (n, 96)
    sub, nosub = committed["status_subgroup"], committed["status_no_subgroup"]
    assert ((nosub == np.where(sub == gen.NOT_IN_SUBGROUP, gen.OK, sub))).all()
    by = lambda f: {int(s) for s, g in zip(sub, fam) if g == f}
    assert by("g1") == by("cleared") == {gen.OK}
    assert by("torsion") == by("torsion_plus_g1") == by("composite") == {gen.NOT_IN_SUBGROUP}
    assert by("x_off_curve") == {gen.NOT_ON_CURVE} and by("encoding") == {gen.BAD_ENCODING, gen.INFINITY}
    assert len(set(committed["records"].tobytes()[48 * i:48 * i + 48] for i in range(n))) >= n - 24   # repeats: (0, +-2) is all of order 3; k and r - k share an x
    # a point is stored exactly where the decoder without the subgroup test owes one
    assert ((committed["points"] != 0).any(axis=1) == (nosub == gen.OK)).all()
    assert os.path.getsize(os.path.join(GOLDEN, "decode_edge_records.npz")) < 128 * 1024


@pytest.mark.parametrize("family", ["g1", "torsion", "torsion_plus_g1", "composite", "cleared", "x_on_curve", "x_off_curve",
                                    "sign_edge", "encoding"])
def test_a_sample_of_every_family_regenerates(gen, committed, family):
    """The first entries of the family, rebuilt (with every self-check of the generator: order of T exactly l,
    [r](T + Q) != inf, [r](h Q) == inf, Euler's criterion, the definitional decoder) == the committed ones."""
    take = {"g1": 12, "torsion": 20, "torsion_plus_g1": 20, "composite": 10, "cleared": 4, "x_on_curve": 14, "x_off_curve": 14,
            "sign_edge": 8, "encoding": 10}[family]
    rows = np.nonzero(committed["family"] == family.encode())[0][:take]
    got = gen.entries(family, take)
    assert len(got) == take == len(rows)
    for i, (rec, st_sub, st_nosub, ptb) in zip(rows, got):
        assert committed["records"][i].tobytes() == rec
        assert (int(committed["status_subgroup"][i]), int(committed["status_no_subgroup"][i])) == (st_sub, st_nosub)
        assert committed["points"][i].tobytes() == ptb


def test_the_sign_edge_points_sit_at_the_threshold(gen, committed, oracle):
    rows = np.nonzero(committed["family"] == b"sign_edge")[0]
    half = (oracle.P - 1) // 2
    ys = {int.from_bytes(committed["points"][i, 48:].tobytes(), "big") for i in rows}
    assert half - 4 in ys and half + 5 in ys and all(abs(y - half) < 16 for y in ys)
    for i in rows:                                                   # the point carries the y its flag asks for
        y = int.from_bytes(committed["points"][i, 48:].tobytes(), "big")
        assert (y > half) == bool(committed["records"][i, 0] & 0x20)


def test_serialisation_is_reproducible(gen, committed):
    arrs = {k: committed[k] for k in ("records", "status_subgroup", "status_no_subgroup", "points", "family")}
    with open(os.path.join(GOLDEN, "decode_edge_records.npz"), "rb") as f:
        assert gen.npz_bytes(arrs) == f.read()
