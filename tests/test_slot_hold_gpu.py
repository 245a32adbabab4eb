"""Every batched entry point gives back what it took: the MSM slot (and the second one the tracker calls borrow), and
its reference on a resident base set or a fixed-base table.

The entry points below hold their slot through one shared helper (SlotHold, csrc/api_helpers.h).  On ONE context, one
call of each at the smallest shape that crosses its structure, in its host and its resident form (the latter on the
slot's stream and on a stream of the caller's), each result against the model or fixture its own test file uses; then
one call of each that is refused for its arguments.  After every call all eight slots are free again
(curdle_msm_free_slots), and in the end eight pipelined MSMs still find eight slots and the ninth is told CURDLE_EBUSY.
Nothing here is timed."""
import os

import numpy as np
import pytest

import fbase_model as fm
import jac_check_cases as jc
from conftest import ROOT
from test_compress_batch_gpu import batch as compress_batch
from test_decode_edges_gpu import Edge
from test_msm_gpu import rand_scalars
from test_normalize_gpu import JAC, XYZZ, batch as normalize_batch, mul_case, pool, products  # noqa: F401  (fixtures)
from test_tracker_batch_gpu import honest, single
from test_tracker_own_gpu import Plant
from test_tracker_prove_gpu import limbs

pytestmark = pytest.mark.gpu

FAKE = 0x7F0000001000          # a multiple of 16 that is never dereferenced: the refusals come before any access
AFF, COMP = 0, 1


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def blank(nbytes):
    import torch
    t = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


def back(t, n, dtype):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype).reshape(n, -1)


def streams():
    """None for the slot's own stream, then a stream of the caller's."""
    import torch
    return (None, torch.cuda.Stream(device="cuda:0").cuda_stream)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert (got == want).all(), (what, np.argwhere(got != want)[:4].tolist())


def all_back(cm, what):
    assert cm.msm_free_slots() == cm.MSM_SLOTS, what


def test_point_families(gpu, oracle, pool, products):
    """Compression (17), normalisation (65: more than one inversion group, both forms), the scalar multiplications
    (17), the affine and the Jacobian check (17) and the one-shot decoding through a slot (17)."""
    cm = gpu
    all_back(cm, "before")
    # compression
    n = 17
    pts, want = compress_batch(oracle, pool, n, 5, {3})
    want = np.frombuffer(b"".join(want), dtype=np.uint8).reshape(n, 48)
    same(cm.g1_compress_batch(pts), want, "compress, host")
    all_back(cm, "compress, host")
    d_in = dev(pts)
    for st in streams():
        d_out = blank(n * 48)
        cm.g1_compress_batch_device(d_in.data_ptr(), n, d_out.data_ptr(), stream=st)
        same(back(d_out, n, np.uint8), want, ("compress, resident", st))
        all_back(cm, ("compress, resident", st))
    # normalisation
    n = 65
    for form in (JAC, XYZZ):
        pts, want = normalize_batch(oracle, pool, n, form, 30 + form, inf_at={40}, dens=("one", "random"))
        a = cm.stat_normalize()
        same(cm.g1_normalize_batch(pts, form), want, ("normalise, host", form))
        b = cm.stat_normalize()
        assert b["points"] - a["points"] == n and b["groups"] - a["groups"] >= 2
        all_back(cm, ("normalise, host", form))
        d_in = dev(pts)
        for st in streams():
            d_out = blank(n * 96)
            cm.g1_normalize_batch_device(d_in.data_ptr(), form, n, d_out.data_ptr(), stream=st)
            same(back(d_out, n, np.uint64), want, ("normalise, resident", form, st))
            all_back(cm, ("normalise, resident", form, st))
    # scalar multiplications: the host form and the resident one
    n = 17
    points, sc, adds, want = mul_case(oracle, products, n, None, True)
    same(cm.g1_scalar_mul_batch(points, sc, adds), want, "scalar-mul, host")
    all_back(cm, "scalar-mul, host")
    d_p, d_sc, d_a = dev(points), dev(sc), dev(adds)
    for st in streams():
        d_out = blank(n * 96)
        cm.g1_scalar_mul_batch_device(d_p.data_ptr(), d_sc.data_ptr(), n, d_a.data_ptr(), n, d_out.data_ptr(), stream=st)
        same(back(d_out, n, np.uint64), want, ("scalar-mul, resident", st))
        all_back(cm, ("scalar-mul, resident", st))
    # the point checks: 17 points spread over the fixture, affine and Jacobian
    z = np.load(os.path.join(ROOT, "tests", "golden", "affine_check_points.npz"))
    cs = jc.cases()
    pick = np.array([i for i in range(cs.n) if cs.kind[i] == "scaled_random"])
    idx = np.linspace(0, len(pick) - 1, 17).astype(int)
    aff, jac = np.ascontiguousarray(z["points"][idx]), np.ascontiguousarray(cs.points[pick[idx]])
    want = z["status_subgroup"][idx]
    assert (cs.want_sub[pick[idx]] == want).all() and len(set(want.tolist())) >= 2
    same(cm.g1_check_batch(aff, True), want, "check, host")
    same(cm.g1_check_jac_batch(jac, True), want, "Jacobian check, host")
    all_back(cm, "checks, host")
    d_aff, d_jac = dev(aff), dev(jac)
    for st in streams():
        same(cm.g1_check_batch_device(d_aff.data_ptr(), 17, True, stream=st), want, ("check, resident", st))
        same(cm.g1_check_jac_batch_device(d_jac.data_ptr(), 17, True, stream=st), want, ("Jacobian check, resident", st))
        all_back(cm, ("checks, resident", st))
    # decoding: without the subgroup test, and with it once the two-step form is out of the way, the call takes a slot
    e = Edge(oracle)
    idx = np.linspace(0, e.n - 1, 17).astype(int)
    blob = e.recs[idx].tobytes()
    got, st = cm.g1_decompress_batch(blob, False)
    same(st, e.st_nosub[idx], "decode statuses"), same(got, e.words[idx], "decoded points")
    with cm.knobs(TWO_KERNEL_MAX=0):
        got, st = cm.g1_decompress_batch(blob, True)
    same(st, e.st_sub[idx], "decode statuses, subgroup")
    same(got, np.where((e.st_sub[idx] == 0)[:, None], e.words[idx], 0), "decoded points, subgroup")
    all_back(cm, "decode")


def test_whisk_families(gpu, oracle, coracle):
    """Tracker proofs verified (k = 3, hashed on the host and on the device, and resident) and generated (k = 3, both
    forms), the ownership search (n = 17, m = 2), the fixed-base multiplication in two passes (n = 257 under
    FBASE_PASS = 256, both output forms) and the tracker batch (n = 3, with and without commitments)."""
    cm = gpu
    all_back(cm, "before")
    # verification: two honest members around one with S + 1
    rand = oracle.Rand(505)
    krs = [(rand.get_fr(), rand.get_fr()) for _ in range(3)]
    ms = [honest(cm, oracle, k, r, 900 + j)[0] for j, (k, r) in enumerate(krs)]
    t, kc, p = ms[1]
    ms[1] = (t, kc, p[:96] + ((int.from_bytes(p[96:], "big") + 1) % oracle.R).to_bytes(32, "big"))
    expected = [single(cm, m) for m in ms]
    assert expected == [1, 0, 1]
    tr, kcs, pr = (list(x) for x in zip(*ms))
    for route, flags in (("host", cm.TRACKER_HASH_HOST), ("device", cm.TRACKER_HASH_DEVICE)):
        a = cm.stat_tracker()
        assert cm.whisk_is_valid_tracker_proof_batch(tr, kcs, pr, flags=flags).tolist() == expected, route
        assert cm.stat_tracker()[route] - a[route] == 3
        all_back(cm, ("verify", route))
    d = [dev(np.frombuffer(b"".join(x), dtype=np.uint8)) for x in (tr, kcs, pr)]
    for st in streams():
        got = cm.whisk_is_valid_tracker_proof_batch_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 3, st or 0)
        assert got.tolist() == expected, st
        all_back(cm, ("verify, resident", st))
    # generation: the rand form draws as three single calls do, and the blinders form is given those draws
    ks = limbs(oracle, [k for k, _ in krs])
    single_rand = cm.Rand(4711)
    want = [cm.whisk_generate_tracker_proof(tr[i], ks[i], single_rand) for i in range(3)]
    proofs, res = cm.whisk_generate_tracker_proof_batch(tr, ks, rand=cm.Rand(4711))
    assert res.tolist() == [cm.OK] * 3 and [x.tobytes() for x in proofs] == want
    all_back(cm, "prove, rand")
    draws = oracle.Rand(4711)
    proofs, res = cm.whisk_generate_tracker_proof_batch(tr, ks, blinders=limbs(oracle, [draws.get_fr() for _ in range(3)]))
    assert res.tolist() == [cm.OK] * 3 and [x.tobytes() for x in proofs] == want
    all_back(cm, "prove, blinders")
    # ownership
    plant = Plant(oracle)
    n, m = 17, 2
    idx = plant.corners(n, m, 1702)
    want = plant.want(idx, m)
    assert want.sum() == 4
    same(cm.whisk_find_own_trackers(plant.records[idx], plant.key_limbs[:m]), want, "own, host")
    all_back(cm, "own, host")
    d_trk, d_ks = dev(plant.records[idx]), dev(plant.key_limbs[:m])
    for st in streams():
        d_out = blank(m * n)
        cm.whisk_find_own_trackers_device(d_trk.data_ptr(), n, d_ks.data_ptr(), m, d_out.data_ptr(), stream=st)
        same(back(d_out, m, np.uint8), want, ("own, resident", st))
        all_back(cm, ("own, resident", st))
    # fixed base: 257 scalars in passes of 256
    fams = fm.digit_families(oracle)
    ks = [k for name in ("small_and_top", "low_zero", "all_ff", "randoms") for _, k in fams[name]][:257]
    n = len(ks)
    assert n == 257
    sc = fm.to_limbs(oracle, ks)
    want = fm.expected_arrays(oracle, coracle, ks)
    d_sc = dev(sc)
    with cm.knobs(FBASE_PASS=256):
        for form, rec, dtype in ((AFF, 96, np.uint64), (COMP, 48, np.uint8)):
            a = cm.stat_fbase()
            same(cm.g1_fixed_base_mul_batch(sc, out_form=form), want[form], ("fixed base, host", form))
            b = cm.stat_fbase()
            assert b["scalars"] - a["scalars"] == n and b["launches"] - a["launches"] == 2
            all_back(cm, ("fixed base, host", form))
            for st in streams():
                d_out = blank(n * rec)
                cm.g1_fixed_base_mul_batch_device(d_sc.data_ptr(), 0, n, d_out.data_ptr(), out_form=form, stream=st)
                same(back(d_out, n, dtype), want[form], ("fixed base, resident", form, st))
                all_back(cm, ("fixed base, resident", form, st))
    same(back(d_sc, n, np.uint64), sc, "the caller's scalars")
    # the tracker batch
    pairs = [(k, r) for (_, k), (_, r) in zip(fm.whisk_scalars(oracle)[4:7], fm.whisk_scalars(oracle)[8:11])]
    ks3, rs3 = fm.to_limbs(oracle, [k for k, _ in pairs]), fm.to_limbs(oracle, [r for _, r in pairs])
    tb = [fm.tracker_bytes(oracle, coracle, k, r) for k, r in pairs]
    want_t = np.frombuffer(b"".join(x for x, _ in tb), dtype=np.uint8).reshape(3, 96)
    want_c = np.frombuffer(b"".join(c for _, c in tb), dtype=np.uint8).reshape(3, 48)
    trk, com = cm.whisk_compute_trackers_batch(ks3, rs3)
    same(trk, want_t, "trackers"), same(com, want_c, "commitments")
    all_back(cm, "trackers with commitments")
    trk, com = cm.whisk_compute_trackers_batch(ks3, rs3, commitments=False)
    assert com is None
    same(trk, want_t, "trackers alone")
    all_back(cm, "trackers alone")


def test_msm_families(gpu, oracle, coracle):
    """curdle_msm_g1_dbases_host over a 33-point set and curdle_msm_g1_multi over two sets of 33."""
    cm = gpu
    all_back(cm, "before")
    k, q = oracle.Rand(33).get_frs(2)
    pts, pts2 = coracle.points_walk(k, q, 33), coracle.points_walk(k + 1, q, 33)
    sc = rand_scalars(np.random.default_rng(33), 33, oracle)
    exp, exp2 = coracle.msm_pippenger(pts, sc, threads=2), coracle.msm_pippenger(pts2, sc, threads=2)
    bases = cm.DBases(pts)
    same(bases.msm_host(sc), exp, "resident bases, host scalars")
    all_back(cm, "resident bases")
    # refused for its count: the set's reference and the slot are back, and the set still works
    out = np.zeros(18, dtype=np.uint64)
    assert cm._msm_dbases_host(bases._h, sc.ctypes.data, 34, out.ctypes.data) == cm.EINVAL and "33 resident bases" in cm.last_error()
    same(bases.msm_host(sc), exp, "resident bases after a refusal")
    bases.free()
    all_back(cm, "resident bases freed")
    got = cm.msm_g1_multi([pts, pts2], sc)
    same(got[0], exp, "multi, set 0"), same(got[1], exp2, "multi, set 1")
    all_back(cm, "multi")


def test_refused_calls_take_nothing(gpu):
    """One call of each family that its argument checks refuse: a resident pointer off a multiple of 16 where the form
    has one to refuse, a count above the family's limit or a null argument otherwise.  Nothing behind the pointers is
    read, no counter moves and every slot stays free."""
    cm = gpu
    E = cm.EINVAL
    stats = lambda: (cm.stat_normalize(), cm.stat_tracker(), cm.stat_tracker_prove(), cm.stat_tracker_own(), cm.stat_fbase())
    before = stats()

    def refused(rc, text):
        assert rc == E and text in cm.last_error(), (rc, text, cm.last_error())
        all_back(cm, text)

    refused(cm._g1_compress_batch(FAKE, (1 << 27) + 1, FAKE), "2^27")
    refused(cm._g1_compress_batch_device(FAKE, (1 << 27) + 1, FAKE, None), "2^27")
    refused(cm._g1_normalize_batch(FAKE, 0, (1 << 24) + 1, FAKE), "2^24")
    refused(cm._g1_normalize_batch_device(FAKE + 8, 0, 17, FAKE, None), "multiples of 16")
    refused(cm._scalar_mul_batch_device(FAKE, FAKE + 8, 17, None, 17, FAKE, None), "multiples of 16")
    refused(cm._scalar_mul_batch(FAKE, FAKE, 1, None, (1 << 24) + 1, FAKE), "2^24")
    refused(cm._check_batch(FAKE, (1 << 27) + 1, 1, FAKE), "2^27")
    refused(cm._check_batch_device(FAKE, (1 << 27) + 1, 1, FAKE, None), "2^27")
    refused(cm._check_jac_batch(FAKE, (1 << 27) + 1, 1, FAKE), "2^27")
    refused(cm._check_jac_batch_device(FAKE, (1 << 27) + 1, 1, FAKE, None), "2^27")
    refused(cm._decompress_batch(FAKE, (1 << 27) + 1, 0, FAKE, FAKE), "2^27")
    res = np.full(3, 77, dtype=np.int32)
    refused(cm._whisk_valid_tracker_batch_ex(FAKE, None, FAKE, 3, cm.TRACKER_HASH_HOST, res.ctypes.data), "null argument")
    assert res.tolist() == [E] * 3
    refused(cm._whisk_valid_tracker_batch_device(None, FAKE, FAKE, 3, res.ctypes.data, None), "null argument")
    proofs = np.full(3 * 128, 77, dtype=np.uint8)
    refused(cm._whisk_gen_tracker_batch_blinders(FAKE, None, FAKE, 3, proofs.ctypes.data, res.ctypes.data), "null argument")
    assert res.tolist() == [E] * 3 and not proofs.any()
    owned = np.zeros((1 << 20) + 1, dtype=np.uint8)
    refused(cm._whisk_find_own(FAKE, (1 << 20) + 1, FAKE, 1, owned.ctypes.data), "2^20")
    assert (owned == cm.TRACKER_UNKNOWN).all()
    refused(cm._whisk_find_own_device(FAKE + 8, 17, FAKE, 2, FAKE, None), "multiples of 16")
    refused(cm._fbase_mul(None, FAKE, None, (1 << 24) + 1, AFF, FAKE), "2^24")
    refused(cm._fbase_mul_device(None, FAKE + 8, None, 257, AFF, FAKE, None), "multiples of 16")
    refused(cm._whisk_compute_trackers_batch(FAKE, FAKE, (1 << 22) + 1, FAKE, FAKE), "2^22")
    assert stats() == before


def test_eight_pipelined_msms_still_find_eight_slots(gpu, oracle, coracle):
    """Runs last in this file, after every call above: eight submits of 32 pairs take one slot each, the ninth is told
    CURDLE_EBUSY, and the eight results are the oracle's."""
    import torch
    cm = gpu
    all_back(cm, "before")
    k, q = oracle.Rand(32).get_frs(2)
    pts = [coracle.points_walk(k + i, q, 32) for i in range(cm.MSM_SLOTS)]
    scs = [rand_scalars(np.random.default_rng(320 + i), 32, oracle) for i in range(cm.MSM_SLOTS)]
    exp = [coracle.msm_pippenger(p, s, threads=2) for p, s in zip(pts, scs)]
    d_p = [torch.from_numpy(p.view(np.int64)).to("cuda:0") for p in pts]
    d_s = [torch.from_numpy(s.view(np.int64)).to("cuda:0") for s in scs]
    torch.cuda.synchronize()
    tickets = [cm.msm_g1_device_submit(d_p[i].data_ptr(), d_s[i].data_ptr(), 32) for i in range(cm.MSM_SLOTS)]
    assert sorted(t & 0x7 for t in tickets) == list(range(cm.MSM_SLOTS))
    assert cm.msm_free_slots() == 0
    with pytest.raises(cm.CurdleError) as e:
        cm.msm_g1_device_submit(d_p[0].data_ptr(), d_s[0].data_ptr(), 32)
    assert e.value.code == cm.EBUSY
    for i, t in enumerate(tickets):
        same(cm.msm_wait(t), exp[i], ("ticket", i))
    all_back(cm, "after the waits")
