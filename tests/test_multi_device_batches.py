"""The batched Whisk and point entry points on a SECOND device context: fixed-base multiplication and the tracker
batch built on it, tracker-proof verification and generation, the ownership search, normalisation, the resident
scalar multiplication, compression, batched transcripts, point decoding and the point checks.

tests/test_multi_device.py drives two contexts through the MSM, curdle_verify* and the Whisk shuffle batch only; the
single-context files of the calls above never leave context 0.  Here every call runs
  * on the calling thread, which is context 0,
  * through on_device(cm, 1, ...), a thread whose current context is 1,
  * and, for the resident forms, over tensors on the context's own HIP device, once on the library's stream and once
    on a torch stream of that device,
and every result is compared bit for bit with the models and fixtures the single-context files use (fbase_model,
tracker_own_model's Plant, tracker_prove_model, merlin_model, the case pools of the tracker, normalise and compress
tests, decode_edge_records.npz, affine_check_points.npz) -- never with context 0's output alone.  Where the library
keeps a curdle_stat_* counter for the call it must move by exactly the members of the call: the device path ran.
(Compression, decoding and the point checks have no host path and no counter.)

With devices = {0, 0} both contexts share one GPU, which proves the slot, stream and table bookkeeping per context;
the last test of tests/test_multi_device.py runs this file again under tools/logical_devices_shim.cpp, where a launch,
copy or event record that mixes the two logical devices fails the call.  The sizes are one wave plus a tail (65 to
300 members; the two fixtures are taken whole, one pass each): the heavy sizes stay in the single-context files."""
import os
import threading

import numpy as np
import pytest

import fbase_model as fm
import jac_check_cases as jc
import merlin_model as mm
import tracker_prove_model as tpm
from conftest import ROOT
from test_compress_batch_gpu import batch as compress_batch, pool as compress_pool, sign_edge_case  # noqa: F401
from test_decode_edges_gpu import Edge
from test_multi_device import DEVS, on_device, two  # noqa: F401  (two: the module-scoped fixture of that file)
from test_normalize_gpu import JAC, XYZZ, batch as normalize_batch, mul_case, pool, products  # noqa: F401
from test_tracker_batch_gpu import pool as tracker_pool, single  # noqa: F401  (the tracker members of that file)
from test_tracker_own_gpu import Plant, launches as own_launches
from test_tracker_prove_gpu import limbs
from test_transcript_batch_gpu import data_for

pytestmark = pytest.mark.gpu

AFF, COMP = 0, 1
CONTEXTS = (0, 1)


def device_of(d):
    return f"cuda:{DEVS[d]}"


def on_context(cm, d, fn):
    """fn() on the calling thread for context 0 (the thread of the test never selects a device), on a thread that
    selected context d otherwise."""
    return fn() if d == 0 else on_device(cm, d, fn)


def resident(a, d):
    """The bytes of `a` in the memory of context d's device, complete before anything else is queued there."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(device_of(d))
    torch.cuda.synchronize(DEVS[d])
    return t


def blank(nbytes, d, fill=0x5A):
    import torch
    t = torch.full((nbytes,), fill, dtype=torch.uint8, device=device_of(d))
    torch.cuda.synchronize(DEVS[d])
    return t


def streams(d):
    """None for the library's own stream of the slot, then a torch stream of context d's device."""
    import torch
    return (None, torch.cuda.Stream(device=device_of(d)).cuda_stream)


def rows(t, n, dtype):
    import torch
    torch.cuda.synchronize(t.device)
    return t.cpu().numpy().view(dtype).reshape(n, -1)


def same(got, want, what=None):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    bad = np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]
    assert bad.size == 0, (what, "%d rows differ, first at %d" % (bad.size, bad[0]))


# ---------------------------------------------------------------------------------------------------------------
# fixed-base multiplication
# ---------------------------------------------------------------------------------------------------------------
class FixedBase:
    """257 scalars of the model's digit families with multipliers for the second half of the calls, and what the model
    says of them for the generator, 7 G and 11 G."""

    def __init__(self, oracle, coracle):
        fams = fm.digit_families(oracle)
        ks = [k for name in ("small_and_top", "low_zero", "all_ff", "randoms") for _, k in fams[name]][:257]
        assert len(ks) == 257
        ks[255] = 0                                                   # an infinity result on each side of the pass boundary
        ks[256] = fm.R - 1
        ms = [k for _, k in fams["randoms"]] + [k for _, k in fams["single_digits"]][:57]
        ms[0] = 0
        self.n, self.ks, self.ms = 257, ks, ms
        self.sc, self.mu = fm.to_limbs(oracle, ks), fm.to_limbs(oracle, ms)
        self.want = {}
        for base in (None, fm.OTHER_BASE, 11):
            for with_m in (False, True):
                prod = [fm.product(k, ms[i] if with_m else None) for i, k in enumerate(ks)]
                self.want[(base, with_m)] = fm.expected_arrays(oracle, coracle, prod, base)
        assert not self.want[(None, False)][0][255].any() and not self.want[(None, True)][0][0].any()

    def host(self, cm, d, handle, base, with_m, form):
        got = on_context(cm, d, lambda: cm.g1_fixed_base_mul_batch(self.sc, self.mu if with_m else None, base=handle, out_form=form))
        same(got, self.want[(base, with_m)][form], ("host", d, base, with_m, form))

    def resident(self, cm, d, handle, base, with_m, form):
        n, rec = self.n, (48 if form == COMP else 96)
        d_sc, d_mu = resident(self.sc, d), resident(self.mu, d)
        for st in streams(d):
            d_out = blank(n * rec + 32, d)
            on_context(cm, d, lambda: cm.g1_fixed_base_mul_batch_device(
                d_sc.data_ptr(), d_mu.data_ptr() if with_m else 0, n, d_out.data_ptr() + 16, base=handle, out_form=form, stream=st))
            out = rows(d_out, 1, np.uint8)[0]
            assert (out[:16] == 0x5A).all() and (out[16 + n * rec:] == 0x5A).all()
            body = out[16: 16 + n * rec].copy()
            got = body.reshape(n, 48) if form == COMP else body.view(np.uint64).reshape(n, 12)
            same(got, self.want[(base, with_m)][form], ("resident", d, base, with_m, form, st))
        same(rows(d_sc, n, np.uint64), self.sc, "the caller's scalars")

    def every_way(self, cm, d, handle, base):
        """Host and resident entry, both output forms, with and without multipliers: 4 host calls and 8 resident
        ones (two streams), two passes each under FBASE_PASS = 256."""
        a = cm.stat_fbase()
        for form in (AFF, COMP):
            for with_m in (False, True):
                self.host(cm, d, handle, base, with_m, form)
                self.resident(cm, d, handle, base, with_m, form)
        b = cm.stat_fbase()
        assert b["scalars"] - a["scalars"] == 12 * self.n and b["launches"] - a["launches"] == 24
        return b["tables"] - a["tables"]


@pytest.fixture(scope="module")
def fixed(oracle, coracle):
    return FixedBase(oracle, coracle)


def test_fixed_base_tables_per_handle_and_context(two, coracle, fixed):
    """The contexts come up afresh, so every table copy is made inside this test: exactly one per (handle, context), on
    first use there, none afterwards; a handle made on either context works on the other; freeing a handle with copies
    on both leaves the generator's table and the other handle working on both."""
    cm = two
    cm.shutdown()
    cm.init_devices(DEVS)
    with cm.knobs(FBASE_PASS=256):
        a = cm.stat_fbase()
        seven = cm.FBase(coracle.scalar_mul_gen(fm.OTHER_BASE))                 # on the calling thread: context 0
        assert cm.stat_fbase()["tables"] - a["tables"] == 1
        assert fixed.every_way(cm, 0, None, None) == 1                          # the generator's, context 0
        assert fixed.every_way(cm, 0, seven, fm.OTHER_BASE) == 0                # made by curdle_fbase_create
        assert fixed.every_way(cm, 1, None, None) == 1                          # the generator's, context 1
        assert fixed.every_way(cm, 1, seven, fm.OTHER_BASE) == 1                # context 0's handle, first use on context 1
        a = cm.stat_fbase()
        eleven = on_device(cm, 1, lambda: cm.FBase(coracle.scalar_mul_gen(11)))  # made on a thread of context 1 ...
        assert cm.stat_fbase()["tables"] - a["tables"] == 1
        assert fixed.every_way(cm, 0, eleven, 11) == 1                          # ... used from context 0
        assert fixed.every_way(cm, 1, eleven, 11) == 0
        for d in CONTEXTS:
            assert fixed.every_way(cm, d, seven, fm.OTHER_BASE) == 0
            assert fixed.every_way(cm, d, None, None) == 0
        seven.free()                                                            # copies on both contexts
        with pytest.raises(ValueError):
            cm.g1_fixed_base_mul_batch(fixed.sc, base=seven)
        a = cm.stat_fbase()
        for d in CONTEXTS:
            fixed.host(cm, d, None, None, True, COMP)
            fixed.host(cm, d, eleven, 11, False, AFF)
            fixed.resident(cm, d, eleven, 11, True, COMP)
        assert cm.stat_fbase()["tables"] == a["tables"]
        eleven.free()
    a = cm.stat_fbase()
    for d in CONTEXTS:                                                          # the default pass: one launch
        fixed.host(cm, d, None, None, False, AFF)
    b = cm.stat_fbase()
    assert b["launches"] - a["launches"] == 2 and b["tables"] == a["tables"]


def test_whisk_compute_trackers_batch(two, oracle, coracle):
    """The Whisk scalars of the model: every named k (0, 1, 2, r - 1, r - 2, lambda, 2^128) against every r, the random
    ones against each other, and k r = 1 -- 146 members, with and without commitments, in passes of 85 and 128."""
    cm = two
    vals = fm.whisk_scalars(oracle)
    pairs = [(k, r) for _, k in vals[:7] for _, r in vals] + [(k, r) for (_, k), (_, r) in zip(vals[7:], vals[8:] + vals[7:8])]
    inv = vals[-1][1]
    pairs.append((inv, pow(inv, -1, oracle.R)))                                     # k r = 1
    n = len(pairs)
    assert n == 146
    ks, rs = fm.to_limbs(oracle, [k for k, _ in pairs]), fm.to_limbs(oracle, [r for _, r in pairs])
    want = [fm.tracker_bytes(oracle, coracle, k, r) for k, r in pairs]
    want_t = np.frombuffer(b"".join(t for t, _ in want), dtype=np.uint8).reshape(n, 96)
    want_c = np.frombuffer(b"".join(c for _, c in want), dtype=np.uint8).reshape(n, 48)
    want_t1 = np.frombuffer(b"".join(fm.tracker_bytes(oracle, coracle, k, 1)[0] for k, _ in pairs), dtype=np.uint8).reshape(n, 96)
    inf = bytes([0xC0]) + bytes(47)
    assert bytes(want_t[0]) == inf + inf and bytes(want_c[0]) == inf                # k = r = 0
    for d in CONTEXTS:
        with cm.knobs(FBASE_PASS=256):
            a = cm.stat_fbase()
            trk, com = on_context(cm, d, lambda: cm.whisk_compute_trackers_batch(ks, rs))
            b = cm.stat_fbase()
            same(trk, want_t, ("trackers", d)), same(com, want_c, ("commitments", d))
            assert b["scalars"] - a["scalars"] == 3 * n and b["launches"] - a["launches"] == (n + 84) // 85 >= 2
            trk, com = on_context(cm, d, lambda: cm.whisk_compute_trackers_batch(ks, rs, commitments=False))
            c = cm.stat_fbase()
            assert com is None
            same(trk, want_t, ("trackers alone", d))
            assert c["scalars"] - b["scalars"] == 2 * n and c["launches"] - b["launches"] == (n + 127) // 128 >= 2
            trk, com = on_context(cm, d, lambda: cm.whisk_compute_trackers_batch(ks, None))   # r = 1
            same(trk, want_t1, ("r = 1", d)), same(com, want_c, ("commitments, r = 1", d))
        a = cm.stat_fbase()
        trk, com = on_context(cm, d, lambda: cm.whisk_compute_trackers_batch(ks, rs))
        b = cm.stat_fbase()
        same(trk, want_t, ("one pass", d)), same(com, want_c, ("one pass", d))
        assert b["launches"] - a["launches"] == 1 and b["tables"] == a["tables"]


# ---------------------------------------------------------------------------------------------------------------
# tracker proofs: verification, generation, ownership
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def members(two, tracker_pool):
    """Every case of the tracker pool between honest neighbours: (members, the answers the pool states)."""
    hon, cases = tracker_pool
    ms, expected = [], []
    for j, (m, want) in enumerate(cases.values()):
        ms += [hon[j % len(hon)][0], m]
        expected += [1, want]
    ms.append(hon[-1][0])
    expected.append(1)
    assert 65 <= len(ms) <= 300 and {0, 1, two.EINVAL} == set(expected)
    assert [single(two, m) for m in ms] == expected                                 # the host's single call agrees
    return ms, expected


def verify_resident(cm, d, ms, st):
    t, kc, p = zip(*ms)
    dev = [resident(np.frombuffer(b"".join(x), dtype=np.uint8), d) for x in (t, kc, p)]
    return on_context(cm, d, lambda: cm.whisk_is_valid_tracker_proof_batch_device(dev[0].data_ptr(), dev[1].data_ptr(),
                                                                                  dev[2].data_ptr(), len(ms), st or 0))


def verify_host(cm, d, ms, flags):
    t, kc, p = zip(*ms)
    return on_context(cm, d, lambda: cm.whisk_is_valid_tracker_proof_batch(list(t), list(kc), list(p), flags=flags))


def test_tracker_proof_verification(two, members):
    cm = two
    ms, expected = members
    k = len(ms)
    for d in CONTEXTS:
        s = cm.stat_tracker()
        # the two routes by flag, then the plain call moved between them by the knob
        routes = [("device", lambda: verify_host(cm, d, ms, cm.TRACKER_HASH_DEVICE)),
                  ("host", lambda: verify_host(cm, d, ms, cm.TRACKER_HASH_HOST))]
        for value, route in ((1, "device"), (0, "host")):
            def plain(value=value):
                with cm.knobs(TRACKER_DEVICE_HASH=value):
                    return verify_host(cm, d, ms, None)
            routes.append((route, plain))
        for st in streams(d):
            routes.append(("device", lambda st=st: verify_resident(cm, d, ms, st)))
        for route, call in routes:
            got = call()
            assert got.dtype == np.int32 and got.tolist() == expected, (d, route)
            s1 = cm.stat_tracker()
            other = "host" if route == "device" else "device"
            assert s1[route] - s[route] == k and s1[other] == s[other] and s1["handed_back"] == s["handed_back"], (d, route)
            s = s1


class Proving:
    """65 members over sixteen distinct (k, r, blinder) triples -- random pairs of the prover's pool, the prover's case
    families (k = 0, 1, r - 1, r = 1, a tracker of two infinities) and the blinders 0, 1, r - 1 -- with one tracker
    that does not decode in the middle; the 128 bytes of each by the model."""

    def __init__(self, oracle):
        model = tpm.Model(oracle)
        rand = oracle.Rand(77)
        triples = [(rand.get_fr(), rand.get_fr(), rand.get_fr()) for _ in range(5)]
        triples += [(k, r, rand.get_fr()) for _, k, r in tpm.case_families(oracle)]
        triples += [(k, r, b) for (k, r, _), b in zip(triples[:3], (0, 1, oracle.R - 1))]
        assert len(triples) == 16
        proofs = [model.proof(*t) for t in triples]
        self.n = 65
        which = [(5 * i + 3) % 16 for i in range(self.n)]
        self.trackers = [model.tracker(*triples[w][:2]) for w in which]
        self.kcomms = [model.k_commitment(*triples[w][:2]) for w in which]
        self.ks = limbs(oracle, [triples[w][0] for w in which])
        self.blinders = limbs(oracle, [triples[w][2] for w in which])
        self.want = [proofs[w] for w in which]
        self.bad_at = 33
        x_ge_p = bytearray(oracle.P.to_bytes(48, "big"))
        x_ge_p[0] |= 0x80
        self.trackers[self.bad_at] = bytes(x_ge_p) + self.trackers[self.bad_at][48:]
        self.want[self.bad_at] = bytes(128)


@pytest.fixture(scope="module")
def proving(oracle):
    return Proving(oracle)


def test_tracker_proof_generation_and_the_other_contexts_verifier(two, proving):
    cm = two
    g = proving
    for d in CONTEXTS:
        a = cm.stat_tracker_prove()
        proofs, res = on_context(cm, d, lambda: cm.whisk_generate_tracker_proof_batch(g.trackers, g.ks, blinders=g.blinders))
        b = cm.stat_tracker_prove()
        assert proofs.shape == (g.n, 128) and res.dtype == np.int32
        assert res.tolist() == [cm.EINVAL if i == g.bad_at else cm.OK for i in range(g.n)]
        got = [p.tobytes() for p in proofs]
        assert got == g.want, [i for i in range(g.n) if got[i] != g.want[i]][:8]
        assert b["device"] + b["host"] - a["device"] - a["host"] == g.n and b["host"] == a["host"]
        # the verifier on the OTHER context accepts every proof (and answers EINVAL for the tracker that does not decode)
        s = cm.stat_tracker()
        ok = on_context(cm, 1 - d, lambda: cm.whisk_is_valid_tracker_proof_batch(g.trackers, g.kcomms, got,
                                                                                 flags=cm.TRACKER_HASH_DEVICE))
        assert ok.tolist() == [cm.EINVAL if i == g.bad_at else 1 for i in range(g.n)]
        assert cm.stat_tracker()["device"] - s["device"] == g.n


@pytest.fixture(scope="module")
def plant(oracle):
    return Plant(oracle)


OWN_SHAPES = [(65, 3), (130, 5)]


@pytest.mark.parametrize("n,m", OWN_SHAPES)
def test_find_own_trackers(two, plant, n, m):
    """Plant.corners; TRACKER_OWN_PAIRS lowered so that the keys take two launches."""
    cm = two
    idx = plant.corners(n, m, 100 * n + m)
    want = plant.want(idx, m)
    assert {(int(j), int(i)) for j, i in zip(*np.nonzero(want))} == {(0, 0), (m - 1, n - 1), (m - 1, 1), (0, n - 2)}
    tc = -(-n // 16) * 16                                        # a key's trackers, padded to whole waves
    pairs = tc * ((m + 1) // 2)                                  # ... and half the keys a launch
    assert own_launches(n, m, pairs) == 2 and own_launches(n, m) == 1
    for d in CONTEXTS:
        with cm.knobs(TRACKER_OWN_PAIRS=pairs):
            a = cm.stat_tracker_own()
            got = on_context(cm, d, lambda: cm.whisk_find_own_trackers(plant.records[idx], plant.key_limbs[:m]))
            b = cm.stat_tracker_own()
            assert got.shape == (m, n) and (got == want).all(), (d, np.argwhere(got != want)[:8])
            assert b["pairs"] - a["pairs"] == n * m and b["launches"] - a["launches"] == 2 and b["bad"] == a["bad"]
            d_trk, d_ks = resident(plant.records[idx], d), resident(plant.key_limbs[:m], d)
            for st in streams(d):
                d_out = blank(16 + m * n + 16, d)
                a = cm.stat_tracker_own()
                on_context(cm, d, lambda: cm.whisk_find_own_trackers_device(d_trk.data_ptr(), n, d_ks.data_ptr(), m,
                                                                             d_out.data_ptr() + 16, stream=st))
                b = cm.stat_tracker_own()
                out = rows(d_out, 1, np.uint8)[0]
                assert (out[:16] == 0x5A).all() and (out[16 + m * n:] == 0x5A).all()
                assert (out[16:16 + m * n].reshape(m, n) == want).all(), (d, st)
                assert b["pairs"] - a["pairs"] == n * m and b["launches"] - a["launches"] == 2
            same(rows(d_ks, m, np.uint64), plant.key_limbs[:m], "the caller's keys")


# ---------------------------------------------------------------------------------------------------------------
# normalisation, resident scalar multiplication, compression
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lane_points", [None, 8])
def test_normalize_batch(two, oracle, pool, lane_points):
    """Both forms, host and resident entry, one zero denominator (with non-zero X and Y) in the batch, under the lane
    rule of the library and the wide one."""
    cm = two
    n = 130
    for form in (JAC, XYZZ):
        pts, want = normalize_batch(oracle, pool, n, form, 40 + form, inf_at={70}, dens=("one", "random"))
        assert int((~want.any(axis=1)).sum()) == 1 and pts[70, :12].any()
        for d in CONTEXTS:
            with cm.knobs(NORMALIZE_LANE_POINTS=lane_points):
                a = cm.stat_normalize()
                same(on_context(cm, d, lambda: cm.g1_normalize_batch(pts, form)), want, ("host", d, form))
                b = cm.stat_normalize()
                assert b["points"] - a["points"] == n and b["groups"] - a["groups"] == (3 if lane_points is None else 1)
                d_in = resident(pts, d)
                for st in streams(d):
                    d_out = blank((n + 2) * 96, d)
                    on_context(cm, d, lambda: cm.g1_normalize_batch_device(d_in.data_ptr(), form, n, d_out.data_ptr() + 96, stream=st))
                    out = rows(d_out, n + 2, np.uint8)
                    assert (out[0] == 0x5A).all() and (out[n + 1] == 0x5A).all()
                    same(out[1:n + 1].copy().view(np.uint64), want, ("resident", d, form, st))
                assert cm.stat_normalize()["points"] - b["points"] == 2 * n


def test_scalar_mul_results_stay_resident_and_are_msm_bases(two, oracle, coracle, products):
    """curdle_g1_scalar_mul_batch_device on each context's device, per-point scalars and addends; the results, still
    resident there, are the bases of curdle_msm_g1_device on the same context -- on the library's streams and on one
    torch stream of that device for both calls."""
    cm = two
    n = 130
    points, sc, adds, want = mul_case(oracle, products, n, None, True)
    rng = np.random.default_rng(5)
    t = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    t[:, 3] &= np.uint64((1 << 62) - 1)                                                # < r
    exp = coracle.msm_pippenger(want, t, threads=4)
    assert int((~want.any(axis=1)).sum()) >= 5                                         # infinities among the bases
    for d in CONTEXTS:
        d_p, d_sc, d_a, d_t = (resident(x, d) for x in (points, sc, adds, t))
        for st in streams(d):
            d_out = blank(n * 96, d, 0)
            a = cm.stat_normalize()
            on_context(cm, d, lambda: cm.g1_scalar_mul_batch_device(d_p.data_ptr(), d_sc.data_ptr(), n, d_a.data_ptr(), n,
                                                                    d_out.data_ptr(), stream=st))
            assert cm.stat_normalize()["points"] - a["points"] == n
            got = on_context(cm, d, lambda: cm.msm_g1_device(d_out.data_ptr(), d_t.data_ptr(), n, stream=st or 0))
            assert (got == exp).all(), (d, st)
            same(rows(d_out, n, np.uint64), want, ("products", d, st))
        same(rows(d_p, n, np.uint64), points, "the caller's points")


def test_compress_batch_with_the_sign_edges(two, oracle, compress_pool):
    """The compress pool (Z = 1, random Z, Z = 0) and every sign-edge point of the decode fixture in its three Jacobian
    forms: 292 points."""
    cm = two
    pts, want = compress_batch(oracle, compress_pool, 130, 21, {7, 129})
    edge_pts, edge_want = sign_edge_case(oracle)
    pts, want = np.concatenate([pts, edge_pts]), want + edge_want
    n = len(want)
    assert n == 292
    want = np.frombuffer(b"".join(want), dtype=np.uint8).reshape(n, 48)
    for d in CONTEXTS:
        same(on_context(cm, d, lambda: cm.g1_compress_batch(pts)), want, ("host", d))
        d_in = resident(pts, d)
        for st in streams(d):
            d_out = blank(n * 48 + 32, d)
            on_context(cm, d, lambda: cm.g1_compress_batch_device(d_in.data_ptr(), n, d_out.data_ptr() + 13, stream=st))
            out = rows(d_out, 1, np.uint8)[0]
            assert (out[:13] == 0x5A).all() and (out[13 + n * 48:] == 0x5A).all()
            same(out[13:13 + n * 48].reshape(n, 48), want, ("resident", d, st))


# ---------------------------------------------------------------------------------------------------------------
# transcripts, decoding, point checks
# ---------------------------------------------------------------------------------------------------------------
def test_transcript_batch_boundary_programs(two):
    cm = two
    k = 65
    for name, program in mm.boundary_programs().items():
        data = data_for(program, k)
        want_ch = np.zeros((k, mm.n_challenges(program), 32), dtype=np.uint8)
        want_st = np.zeros((k, mm.STATE_SIZE), dtype=np.uint8)
        for i in range(k):
            mc, _, mst, status, _ = mm.run_program(program, bytes(data[i]), mm.BOUNDARY_LABEL)
            assert status == 0
            want_ch[i] = np.frombuffer(b"".join(mc), dtype=np.uint8).reshape(-1, 32)
            want_st[i] = np.frombuffer(mst, dtype=np.uint8)
        for d in CONTEXTS:
            for lanes in (None, 5):                               # one member per wave at this size; ragged waves of five
                a = cm.stat_transcript()
                with cm.knobs(TRANSCRIPT_LANES=lanes):
                    ch, st, status = on_context(cm, d, lambda: cm.transcript_batch(program, data, label=mm.BOUNDARY_LABEL))
                b = cm.stat_transcript()
                assert not status.any(), (name, d, lanes)
                same(ch, want_ch, (name, d, lanes, "challenges")), same(st, want_st, (name, d, lanes, "states"))
                assert b["members"] - a["members"] == k and b["handed_back"] == a["handed_back"]


def test_decode_edge_fixture_one_pass(two, oracle):
    """curdle_g1_decompress_batch and the begin / finish form over the 460 records of the decode fixture."""
    cm = two
    e = Edge(oracle)
    blob = e.recs.tobytes()
    blanked = np.where((e.st_sub == 0)[:, None], e.words, 0)      # the one-shot form hands back zeros for what it rejects
    for d in CONTEXTS:
        pts, st = on_context(cm, d, lambda: cm.g1_decompress_batch(blob, True))
        assert (st == e.st_sub).all(), (d, np.nonzero(st != e.st_sub)[0][:8])
        same(pts, blanked, ("one-shot", d))
        pts, st = on_context(cm, d, lambda: cm.g1_decompress_batch(blob, False))
        assert (st == e.st_nosub).all(), d
        same(pts, e.words, ("no subgroup test", d))

        def two_step():
            pts, pre, ticket = cm.g1_decompress_begin(blob)
            return pts, pre, cm.g1_decompress_finish(ticket, e.n)
        pts, pre, st = on_context(cm, d, two_step)
        assert (pre == e.st_nosub).all() and (st == e.st_sub).all(), d
        same(pts, e.words, ("begin / finish", d))
    # a ticket names its context: begun on context 1, finished from the calling thread
    pts, pre, ticket = on_device(cm, 1, lambda: cm.g1_decompress_begin(blob))
    assert (cm.g1_decompress_finish(ticket, e.n) == e.st_sub).all()
    same(pts, e.words, "begun on context 1")


def test_point_checks_one_pass(two):
    """curdle_g1_check_batch over affine_check_points.npz and curdle_g1_check_jac_batch over the same 555 points in
    Jacobian form with a random Z (tests/jac_check_cases.py), host and resident entry, with and without the subgroup
    test."""
    cm = two
    z = np.load(os.path.join(ROOT, "tests", "golden", "affine_check_points.npz"))
    aff = z["points"]
    cs = jc.cases()
    pick = np.array([i for i in range(cs.n) if cs.kind[i] == "scaled_random"])
    assert len(pick) == len(aff) == 555 and (cs.want_sub[pick] == z["status_subgroup"]).all()
    jac = np.ascontiguousarray(cs.points[pick])
    for d in CONTEXTS:
        d_aff, d_jac = resident(aff, d), resident(jac, d)
        for sub, key in ((True, "status_subgroup"), (False, "status_no_subgroup")):
            want = z[key]
            assert (on_context(cm, d, lambda: cm.g1_check_batch(aff, sub)) == want).all(), (d, sub)
            assert (on_context(cm, d, lambda: cm.g1_check_jac_batch(jac, sub)) == want).all(), (d, sub)
            for st in streams(d):
                got = on_context(cm, d, lambda: cm.g1_check_batch_device(d_aff.data_ptr(), len(aff), sub, stream=st))
                assert (got == want).all(), (d, sub, st)
                got = on_context(cm, d, lambda: cm.g1_check_jac_batch_device(d_jac.data_ptr(), len(jac), sub, stream=st))
                assert (got == want).all(), (d, sub, st)


# ---------------------------------------------------------------------------------------------------------------
# both contexts at once
# ---------------------------------------------------------------------------------------------------------------
def test_both_contexts_at_once_beside_an_msm(two, oracle, coracle, fixed, members, plant):
    """One thread per context runs the fixed-base call (host and resident), the device-hashed tracker verification and
    the ownership search three times each while a third thread runs 4,096-pair MSMs on context 0: every result exact,
    and the counters moved by exactly what the six rounds hold."""
    import torch
    cm = two
    ms, expected = members
    n_own, m_own = OWN_SHAPES[1]
    idx = plant.corners(n_own, m_own, 7)
    own_want = plant.want(idx, m_own)
    k, q = oracle.Rand(1).get_frs(2)
    pts = coracle.points_walk(k, q, 4096)
    rng = np.random.default_rng(4096)
    t = rng.integers(0, 1 << 64, size=(4096, 4), dtype=np.uint64)
    t[:, 3] &= np.uint64((1 << 62) - 1)
    exp = coracle.msm_pippenger(pts, t, threads=4)
    seven = cm.FBase(coracle.scalar_mul_gen(fm.OTHER_BASE))
    for d in CONTEXTS:                                            # the copies of 7 G's table, before the counters are read
        fixed.host(cm, d, seven, fm.OTHER_BASE, False, AFF)
    d_sc = [resident(fixed.sc, d) for d in CONTEXTS]
    d_out = [blank(fixed.n * 48, d, 0) for d in CONTEXTS]
    errors, gate, msms = [], threading.Barrier(3), []
    before = (cm.stat_fbase(), cm.stat_tracker(), cm.stat_tracker_own())

    def worker(d):
        try:
            cm.set_device(d)
            gate.wait()
            for r in range(3):
                if (d + r) % 2:
                    same(cm.g1_fixed_base_mul_batch(fixed.sc, fixed.mu, out_form=COMP), fixed.want[(None, True)][COMP], (d, r))
                else:
                    same(cm.g1_fixed_base_mul_batch(fixed.sc, base=seven), fixed.want[(fm.OTHER_BASE, False)][AFF], (d, r))
                cm.g1_fixed_base_mul_batch_device(d_sc[d].data_ptr(), 0, fixed.n, d_out[d].data_ptr(), base=seven, out_form=COMP)
                same(rows(d_out[d], fixed.n, np.uint8), fixed.want[(fm.OTHER_BASE, False)][COMP], (d, r, "resident"))
                d_out[d].zero_()
                torch.cuda.synchronize(DEVS[d])
                tt, kc, p = zip(*ms)
                got = cm.whisk_is_valid_tracker_proof_batch(list(tt), list(kc), list(p), flags=cm.TRACKER_HASH_DEVICE)
                assert got.tolist() == expected, (d, r)
                got = cm.whisk_find_own_trackers(plant.records[idx], plant.key_limbs[:m_own])
                assert (got == own_want).all(), (d, r)
        except BaseException as e:  # noqa: BLE001 - reported by the test's thread
            errors.append((d, e))
            gate.abort()

    def msm_worker():
        try:
            cm.set_device(0)
            gate.wait()
            for _ in range(3):
                msms.append(cm.msm_g1(pts, t))
        except BaseException as e:  # noqa: BLE001
            errors.append(("msm", e))
            gate.abort()

    threads = [threading.Thread(target=worker, args=(d,)) for d in CONTEXTS] + [threading.Thread(target=msm_worker)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    seven.free()
    assert not errors, errors
    assert len(msms) == 3 and all((got == exp).all() for got in msms)
    fb, tr, own = cm.stat_fbase(), cm.stat_tracker(), cm.stat_tracker_own()
    assert fb["scalars"] - before[0]["scalars"] == 12 * fixed.n and fb["tables"] == before[0]["tables"]
    assert tr["device"] - before[1]["device"] == 6 * len(ms) and tr["host"] == before[1]["host"]
    assert own["pairs"] - before[2]["pairs"] == 6 * n_own * m_own
