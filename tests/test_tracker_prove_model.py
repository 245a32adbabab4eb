"""tests/tracker_prove_model.py held byte for byte against the single call (curdle_whisk_generate_tracker_proof, host
code) over the case families the GPU tests of the batched generator use.  The single call draws its blinder from a
Rand; the model takes the same value as oracle.Rand(seed).get_fr(), the proof's first draw."""
import numpy as np
import pytest

import tracker_prove_model as tpm


@pytest.fixture(scope="module")
def model(oracle):
    return tpm.Model(oracle)


def fr_limbs(oracle, k):
    return np.array(oracle.fr_to_mont_limbs(k % oracle.R), dtype=np.uint64)


def test_the_model_is_the_single_call(cm, oracle, model):
    for j, (name, k, r) in enumerate(tpm.case_families(oracle)):
        seed = 900 + j
        got = cm.whisk_generate_tracker_proof(model.tracker(k, r), fr_limbs(oracle, k), cm.Rand(seed))
        b = oracle.Rand(seed).get_fr()
        assert got == model.proof(k, r, b), name
        assert cm.whisk_is_valid_tracker_proof(model.tracker(k, r), model.k_commitment(k, r), got), name


def test_the_model_on_the_blinders_no_rand_draws(cm, oracle, model):
    """b = 0 (A and B at infinity, s = -c k), 1 and r - 1: no seed draws these, so the model stands alone here -- and
    the verifier, which accepts what it produces."""
    _, k, r = tpm.case_families(oracle)[0]
    inf = oracle.compress(None)
    for b in (0, 1, oracle.R - 1):
        p = model.proof(k, r, b)
        if b == 0:
            assert p[:96] == inf + inf
        if b == 1:
            assert p[:48] == oracle.compress(oracle.G1) and p[48:96] == model.tracker(k, r)[:48]
        assert cm.whisk_is_valid_tracker_proof(model.tracker(k, r), model.k_commitment(k, r), p), b
