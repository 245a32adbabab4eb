"""The oblivious gather over 32-byte records on the GPU (curdle_fr_permute_ct / _device, k_fr_permute_ct): both forms are
held to numpy's a[perm] byte for byte at n = 1 ... 4,096 -- one lane, one wave and one block and their neighbours, and
the cap -- over records of random bytes with an all-ones and an all-zero record among them (the gather knows nothing of
the field), with perm the identity, the reversal, a transposition, random permutations, and gathers that are no
permutations: every entry equal, and entries of n and 0xFFFFFFFF, which give zero records.  The resident form writes
between guard bytes, on the library's stream and on a caller's, and leaves its input alone; 4,097 is refused; the
counter moves by (n, 1) per completed call.  k_g1_permute_ct, which now shares the gather's body, still permutes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 4096)


def records(n, rng):
    rec = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    rec[0] = 0xFF
    if n > 1:
        rec[n - 1] = 0
    return rec


def perms(n, rng):
    ident = np.arange(n, dtype=np.uint32)
    swap = ident.copy()
    swap[0], swap[n - 1] = n - 1, 0
    out = {"identity": ident, "reversal": ident[::-1].copy(), "transposition": swap,
           "random": rng.permutation(n).astype(np.uint32), "random2": rng.permutation(n).astype(np.uint32),
           "all first": np.zeros(n, dtype=np.uint32), "all last": np.full(n, n - 1, dtype=np.uint32)}
    beyond = rng.permutation(n).astype(np.uint32)       # entries at and above n: zero records
    beyond[::3] = n
    beyond[1::5] = 0xFFFFFFFF
    out["beyond"] = beyond
    out["all beyond"] = np.full(n, n, dtype=np.uint32)
    return out


def expected(rec, perm):
    n = len(rec)
    ext = np.vstack([rec, np.zeros((1, 32), dtype=np.uint8)])
    return ext[np.where(perm < n, perm, n)]             # numpy's a[perm], an entry at or above n taking the zero record


@pytest.mark.parametrize("n", SIZES)
def test_both_forms_against_numpy(gpu, n):
    import torch
    rng = np.random.default_rng(n)
    rec = records(n, rng)
    caller = torch.cuda.Stream()
    d_in = torch.from_numpy(rec.reshape(-1).copy()).to("cuda:0")
    for name, perm in perms(n, rng).items():
        want = expected(rec, perm)
        before = gpu.stat_fr_permute_ct()
        got = gpu.fr_permute_ct(rec.view(np.uint64), perm)
        assert (got.view(np.uint8) == want).all(), (n, name, "host form")
        d_perm = torch.from_numpy(perm.view(np.int32)).to("cuda:0")
        for stream in (0, caller.cuda_stream):
            d_out = torch.full((32 * n + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            gpu.fr_permute_ct_device(d_in.data_ptr(), d_perm.data_ptr(), n, d_out.data_ptr() + 16, stream=stream)
            out = d_out.cpu().numpy()
            assert (out[:16] == 0x5A).all() and (out[16 + 32 * n:] == 0x5A).all(), (n, name, stream)
            assert (out[16:16 + 32 * n].reshape(n, 32) == want).all(), (n, name, stream)
        after = gpu.stat_fr_permute_ct()
        assert (after["records"] - before["records"], after["launches"] - before["launches"]) == (3 * n, 3)
        assert (d_perm.cpu().numpy().view(np.uint32) == perm).all()
    assert (d_in.cpu().numpy().reshape(n, 32) == rec).all()


def test_4097_is_refused_with_the_guards_intact(gpu):
    import torch
    n = 4097
    rec = np.random.default_rng(n).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    perm = np.arange(n, dtype=np.uint32)
    d_in = torch.from_numpy(rec.view(np.int64).reshape(-1)).to("cuda:0")
    d_perm = torch.from_numpy(perm.view(np.int32)).to("cuda:0")
    d_out = torch.full((32 * n + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    before = gpu.stat_fr_permute_ct()
    with pytest.raises(gpu.CurdleError) as e:
        gpu.fr_permute_ct_device(d_in.data_ptr(), d_perm.data_ptr(), n, d_out.data_ptr() + 16)
    assert e.value.code == gpu.EINVAL and "4,096" in e.value.msg
    with pytest.raises(gpu.CurdleError) as e:
        gpu.fr_permute_ct(rec, perm)
    assert e.value.code == gpu.EINVAL and "4,096" in e.value.msg
    # overlapping and misaligned records are refused too, with a device present
    for d_o in (d_in.data_ptr() + 32, d_out.data_ptr() + 8):
        with pytest.raises(gpu.CurdleError) as e:
            gpu.fr_permute_ct_device(d_in.data_ptr(), d_perm.data_ptr(), 4, d_o)
        assert e.value.code == gpu.EINVAL
    assert (d_out.cpu().numpy() == 0x5A).all()
    assert gpu.stat_fr_permute_ct() == before


@pytest.mark.parametrize("n", (65, 257))
def test_the_point_gather_shares_the_body_and_still_permutes(gpu, n):
    import torch
    rng = np.random.default_rng(n)
    rec = rng.integers(0, 1 << 64, size=(n, 12), dtype=np.uint64)
    d_in = torch.from_numpy(rec.view(np.int64).reshape(-1)).to("cuda:0")
    for perm in (np.arange(n, dtype=np.uint32)[::-1].copy(), rng.permutation(n).astype(np.uint32),
                 np.full(n, n - 1, dtype=np.uint32)):
        d_perm = torch.from_numpy(perm.view(np.int32)).to("cuda:0")
        d_out = torch.full((96 * n + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        gpu.g1_permute_ct_device(d_in.data_ptr(), d_perm.data_ptr(), n, d_out.data_ptr() + 16)
        out = d_out.cpu().numpy()
        assert (out[:16] == 0x5A).all() and (out[16 + 96 * n:] == 0x5A).all()
        assert (out[16:16 + 96 * n].copy().view(np.uint64).reshape(n, 12) == rec[perm]).all()
