"""The batched oblivious gather on the GPU (curdle_fr_permute_ct_batch / _batch_device, curdle_g1_permute_ct_batch_device,
k_permute_ct_seg): k members of one n in one launch, held to numpy's a[perm] per member byte for byte, at both record
sizes, for n = 1 ... 257 (one lane, one wave, one block and their neighbours) x k = 1, 2, 3, 5 and once at the cap of
n with k = 2.  Records are distinct across members, so a read into a neighbour's segment shows; the entries are the
identity, the reversal, random permutations, every entry equal, and entries of n and 0xFFFFFFFF in member 0 and in the
last member, which must give ZERO records and not member j +- 1's.  The resident forms write between guard bytes, on the
library's stream and on a caller's, and leave their input alone; every refusal is checked; the counter moves by
(k n, 1); the single-permutation kernels still give their bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(n, k) for n in (1, 2, 3, 63, 64, 65, 257) for k in (1, 2, 3, 5)] + [(4096, 2)]


def records(n, k, size, rng):
    """k n records of `size` bytes, every one distinct: random bytes with the flat index in front."""
    rec = rng.integers(0, 256, size=(k * n, size), dtype=np.uint8)
    rec[:, :4] = np.arange(1, k * n + 1, dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    return rec


def entry_sets(n, k, rng):
    ident = np.tile(np.arange(n, dtype=np.uint32), k)
    out = {"identity": ident,
           "reversal": np.tile(np.arange(n, dtype=np.uint32)[::-1], k),
           "random": np.concatenate([rng.permutation(n) for _ in range(k)]).astype(np.uint32),
           "random2": np.concatenate([rng.permutation(n) for _ in range(k)]).astype(np.uint32),
           "all equal": np.repeat(rng.integers(0, n, size=k), n).astype(np.uint32)}
    for name, member in (("beyond in member 0", 0), ("beyond in the last member", k - 1)):
        e = out["random"].copy()
        seg = e[member * n:(member + 1) * n]
        seg[::3] = n                      # one past the segment: the next member's first record, were the index flat
        seg[1::4] = 0xFFFFFFFF            # and the previous member's last
        if n > 2:
            seg[2] = n + 1
        out[name] = e
    return out


def expected(rec, entries, n, k):
    size = rec.shape[1]
    want = np.zeros_like(rec)
    for j in range(k):
        seg = np.vstack([rec[j * n:(j + 1) * n], np.zeros((1, size), dtype=np.uint8)])
        e = entries[j * n:(j + 1) * n]
        want[j * n:(j + 1) * n] = seg[np.where(e < n, e, n)]
    return want


@pytest.mark.parametrize("n,k", SHAPES)
def test_both_record_sizes_against_numpy(gpu, n, k):
    import torch
    rng = np.random.default_rng(1000 * n + k)
    caller = torch.cuda.Stream()
    sets = entry_sets(n, k, rng)
    if n == 4096:  # the cap once: a random gather and the entries beyond, not every pattern
        sets = {name: sets[name] for name in ("random", "beyond in member 0", "beyond in the last member")}
    for size, device_form in ((32, gpu.fr_permute_ct_batch_device), (96, gpu.g1_permute_ct_batch_device)):
        rec = records(n, k, size, rng)
        d_in = torch.from_numpy(rec.reshape(-1).copy()).to("cuda:0")
        nbytes = size * n * k
        for name, entries in sets.items():
            want = expected(rec, entries, n, k)
            before = gpu.stat_fr_permute_ct()
            calls = 0
            if size == 32:
                got = gpu.fr_permute_ct_batch(rec.view(np.uint64), entries, n, k)
                assert (got.view(np.uint8).reshape(k * n, 32) == want).all(), (n, k, name, "host form")
                calls += 1
            d_perm = torch.from_numpy(entries.view(np.int32)).to("cuda:0")
            for stream in (0, caller.cuda_stream):
                d_out = torch.full((nbytes + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                device_form(d_in.data_ptr(), d_perm.data_ptr(), n, k, d_out.data_ptr() + 16, stream=stream)
                out = d_out.cpu().numpy()
                assert (out[:16] == 0x5A).all() and (out[16 + nbytes:] == 0x5A).all(), (n, k, size, name, stream)
                assert (out[16:16 + nbytes].reshape(k * n, size) == want).all(), (n, k, size, name, stream)
                calls += size == 32
            after = gpu.stat_fr_permute_ct()
            assert (after["records"] - before["records"], after["launches"] - before["launches"]) == (calls * k * n, calls)
            assert (d_perm.cpu().numpy().view(np.uint32) == entries).all()
        assert (d_in.cpu().numpy().reshape(k * n, size) == rec).all()


def test_refusals_in_order_with_the_guards_intact(gpu):
    import torch
    rng = np.random.default_rng(7)
    n, k = 8, 3
    rec = rng.integers(0, 1 << 64, size=(k * n, 12), dtype=np.uint64)
    d_in = torch.from_numpy(rec.view(np.int64).reshape(-1)).to("cuda:0")
    d_perm = torch.zeros(4096 * 2, dtype=torch.int32, device="cuda:0")
    d_out = torch.full((96 * n * k + 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    before = gpu.stat_fr_permute_ct()
    i, p, o = d_in.data_ptr(), d_perm.data_ptr(), d_out.data_ptr() + 16

    def refused(call, *args, text=None):
        with pytest.raises(gpu.CurdleError) as e:
            call(*args)
        assert e.value.code == gpu.EINVAL
        if text:
            assert text in e.value.msg, e.value.msg

    for form in (gpu.fr_permute_ct_batch_device, gpu.g1_permute_ct_batch_device):
        # nothing to do comes before everything: no pointer is looked at
        form(0, 0, 0, 5, 0)
        form(0, 0, 5, 0, 0)
        refused(form, 0, p, n, k, o, text="null")
        refused(form, i, 0, n, k, o, text="null")
        refused(form, i, p, n, k, 0, text="null")
        refused(form, 0, p, 4097, 4097, o, text="null")          # null before n
        refused(form, i, p, 4097, 4097, o, text="4,096 records")  # n before k
        refused(form, i, p, n, 4097, o, text="4,096 members")
        refused(form, i, p, 4096, 257, o, text="2^20")            # k n last of the sizes
        refused(form, i, p, 4096, 257, o + 8, text="2^20")        # ... and before the alignment
        refused(form, i, p, n, k, o + 8, text="multiples of 16")
        refused(form, i + 8, p, n, k, o, text="multiples of 16")
        refused(form, i, p + 2, n, k, o, text="multiple of 4")
        refused(form, i, p, n, k, i + 32, text="overlap")
    host = np.zeros((k * n, 4), dtype=np.uint64)
    refused(gpu.fr_permute_ct_batch, np.zeros((4097 * 2, 4), dtype=np.uint64), np.zeros(4097 * 2, dtype=np.uint32), 4097, 2,
            text="4,096 records")
    refused(gpu.fr_permute_ct_batch, np.zeros((4097, 4), dtype=np.uint64), np.zeros(4097, dtype=np.uint32), 1, 4097,
            text="4,096 members")
    assert gpu.fr_permute_ct_batch(host[:0], np.zeros(0, dtype=np.uint32), 0, 7).shape == (0, 4)
    assert (d_out.cpu().numpy() == 0x5A).all()
    assert gpu.stat_fr_permute_ct() == before


@pytest.mark.parametrize("n", (65, 257))
def test_the_single_gathers_keep_their_bits(gpu, n):
    import torch
    rng = np.random.default_rng(n)
    perm = rng.permutation(n).astype(np.uint32)
    perm[5] = n                                           # a zero record in the 32-byte form
    rec = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    want = np.vstack([rec, np.zeros((1, 4), dtype=np.uint64)])[np.where(perm < n, perm, n)]
    assert (gpu.fr_permute_ct(rec, perm) == want).all()
    assert (gpu.fr_permute_ct_batch(rec, perm, n, 1) == want).all()
    pts = rng.integers(0, 1 << 64, size=(n, 12), dtype=np.uint64)
    perm = rng.permutation(n).astype(np.uint32)
    d_in = torch.from_numpy(pts.view(np.int64).reshape(-1)).to("cuda:0")
    d_perm = torch.from_numpy(perm.view(np.int32)).to("cuda:0")
    d_out = torch.zeros(12 * n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    gpu.g1_permute_ct_device(d_in.data_ptr(), d_perm.data_ptr(), n, d_out.data_ptr())
    assert (d_out.cpu().numpy().view(np.uint64).reshape(n, 12) == pts[perm]).all()
