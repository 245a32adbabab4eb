"""CURDLE_SHUFFLE_CONSTANT_TIME on the GPU: the flagged curdle_shuffle_permute_commit_ex against the call without flags,
byte for byte on Ts, Us, M, rs_m and on the next draw from rand; the counters prove which kernels ran (one launch of
k_g1_mul_ct over 2 ell records, two walks and one sum of the constant-time MSM over ell + 4 terms, no normalisation
kernel); the oblivious gather alone between guard bytes; the cap; and the flagged outputs through curdle_prove and
curdle_verify.  The walk's two scalar forms both run here: the permutation as plain uint32, the blinders as fr.Elements."""
import numpy as np
import pytest

import msm_ct_model as mm

pytestmark = pytest.mark.gpu

CT = 1
_setups = {}


def setup(cm, ell):
    """(crs, Rs, Ss) for ell, made once."""
    if ell not in _setups:
        rand = cm.Rand(ell)
        crs = cm.CRS(ell, rand)
        _setups[ell] = (crs, rand.get_g1_affines(ell), rand.get_g1_affines(ell))
    return _setups[ell]


def perms(cm, ell):
    ident = np.arange(ell, dtype=np.uint32)
    swap = ident.copy()
    swap[[0, ell - 1]] = swap[[ell - 1, 0]]
    return {"identity": ident, "reversal": ident[::-1].copy(), "transposition": swap,
            "random": cm.Rand(1000 + ell).generate_permutation(ell)}


def scalars(oracle):
    return {"0": 0, "1": 1, "r-1": mm.R - 1, "random": oracle.Rand(77).get_fr()}


def stats(cm):
    return cm.stat_msm_ct(), cm.stat_g1_mul_ct(), cm.stat_normalize()


def step(cm, crs, Rs, Ss, perm, k, flags, seed=5):
    rand = cm.Rand(seed)
    Ts, Us, M, rs_m = cm.shuffle_permute_commit(crs, Rs, Ss, perm, k, rand, flags=flags)
    return Ts, Us, M, rs_m, rand.get_frs(2)


def compare(cm, oracle, ell, perm, k_int, Rs=None, name=""):
    crs, R0, Ss = setup(cm, ell)
    Rs = R0 if Rs is None else Rs
    k = np.array(oracle.fr_to_mont_limbs(k_int), dtype=np.uint64)
    want = step(cm, crs, Rs, Ss, perm, k, None)
    before = stats(cm)
    got = step(cm, crs, Rs, Ss, perm, k, CT)
    after = stats(cm)
    for a, b, what in zip(got, want, ("Ts", "Us", "M", "rs_m", "the next draws")):
        assert a.shape == b.shape and (a == b).all(), (name, ell, what)
    d = {key: after[0][key] - before[0][key] for key in after[0]}
    assert d == {"pairs": ell + 4, "walks": 2, "sums": 1}, (name, d)
    assert (after[1]["scalars"] - before[1]["scalars"], after[1]["launches"] - before[1]["launches"]) == (2 * ell, 1), name
    assert after[2] == before[2], name                                       # no normalisation kernel
    zero = step(cm, crs, Rs, Ss, perm, k, 0)                                 # flags = 0 is the call without flags
    assert all((a == b).all() for a, b in zip(zero, want)) and stats(cm)[:2] == after[:2], name
    return got


@pytest.mark.parametrize("ell", [4, 12])
def test_every_permutation_with_every_scalar(gpu, oracle, ell):
    for pname, perm in perms(gpu, ell).items():
        for kname, k in scalars(oracle).items():
            compare(gpu, oracle, ell, perm, k, name="%s, k = %s" % (pname, kname))


@pytest.mark.parametrize("ell", [60, 124])
def test_permutations_and_scalars(gpu, oracle, ell):
    ps, ks = perms(gpu, ell), scalars(oracle)
    for pname, perm in ps.items():
        compare(gpu, oracle, ell, perm, ks["random"], name=pname)
    for kname in ("0", "1", "r-1"):
        compare(gpu, oracle, ell, ps["random"], ks[kname], name="k = " + kname)


def test_ell_508_once(gpu, oracle):
    compare(gpu, oracle, 508, perms(gpu, 508)["random"], scalars(oracle)["random"], name="508")


def test_an_r_at_infinity(gpu, oracle):
    ell = 12
    _, Rs, _ = setup(gpu, ell)
    Rs = Rs.copy()
    Rs[1] = 0
    Rs[ell - 1] = 0
    Ts = compare(gpu, oracle, ell, perms(gpu, ell)["random"], scalars(oracle)["random"], Rs=Rs, name="R at infinity")[0]
    assert int((~Ts.any(axis=1)).sum()) == 2


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_the_gather_alone_between_guard_bytes(gpu, n):
    import torch
    rng = np.random.default_rng(n)
    rec = rng.integers(0, 1 << 64, size=(n, 12), dtype=np.uint64)
    for perm in (np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)[::-1].copy(), rng.permutation(n).astype(np.uint32),
                 np.zeros(n, dtype=np.uint32), np.full(n, n - 1, dtype=np.uint32)):       # the last two are no permutations: a gather
        d_in = torch.from_numpy(rec.view(np.int64).reshape(-1)).to("cuda:0")
        d_perm = torch.from_numpy(perm.view(np.int32)).to("cuda:0")
        d_out = torch.full((96 * n + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        gpu.g1_permute_ct_device(d_in.data_ptr(), d_perm.data_ptr(), n, d_out.data_ptr() + 16)
        out = d_out.cpu().numpy()
        assert (out[:16] == 0x5A).all() and (out[16 + 96 * n:] == 0x5A).all()
        assert (out[16:16 + 96 * n].copy().view(np.uint64).reshape(n, 12) == rec[perm]).all()
        assert (d_in.cpu().numpy().view(np.uint64).reshape(n, 12) == rec).all()
        assert (d_perm.cpu().numpy().view(np.uint32) == perm).all()
    with pytest.raises(gpu.CurdleError) as e:
        gpu.g1_permute_ct_device(d_in.data_ptr(), d_perm.data_ptr(), 4097, d_out.data_ptr() + 16)
    assert e.value.code == gpu.EINVAL and "4,096" in e.value.msg


def test_4097_is_refused(gpu):
    """The cap of the flagged step: before any device work and before anything is drawn."""
    from test_msm_ct_abi import _fns
    _, _, raw = _fns(gpu)
    crs, Rs, Ss = setup(gpu, 4)
    out = np.full(4 * 12 * 2 + 18 + 16, 77, dtype=np.uint64)
    perm, k = np.arange(4097, dtype=np.uint32), np.zeros(4, dtype=np.uint64)
    before = stats(gpu)
    r1 = gpu.Rand(9)
    nxt = gpu.Rand(9).get_frs(1)
    rc = raw(crs._h, Rs.ctypes.data, Ss.ctypes.data, 4097, perm.ctypes.data, k.ctypes.data, r1._h, CT, out[:48].ctypes.data,
             out[48:96].ctypes.data, out[96:114].ctypes.data, out[114:].ctypes.data)
    assert rc == gpu.EINVAL and "4,096" in gpu.last_error()
    assert (out == 77).all() and (r1.get_frs(1) == nxt).all() and stats(gpu) == before


def test_the_flagged_outputs_prove_and_verify(gpu, oracle):
    ell = 60
    crs, Rs, Ss = setup(gpu, ell)
    perm = perms(gpu, ell)["random"]
    k = np.array(oracle.fr_to_mont_limbs(scalars(oracle)["random"]), dtype=np.uint64)
    Ts, Us, M, rs_m = gpu.shuffle_permute_commit(crs, Rs, Ss, perm, k, gpu.Rand(5), flags=CT)
    proof = gpu.prove(crs, Rs, Ss, Ts, Us, M, perm, k, rs_m, gpu.Rand(42))
    assert gpu.verify(crs, proof, Rs, Ss, Ts, Us, M, gpu.Rand(43)) is True
    assert gpu.verify(crs, proof, Rs, Ss, Us, Ts, M, gpu.Rand(43)) is False
