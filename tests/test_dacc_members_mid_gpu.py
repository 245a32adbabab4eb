"""curdle_dacc_run_members at mid sizes and on skewed rows, bit for bit against the member model and the C oracle: the five
shapes of dacc_members_model.mid_cases -- 2 x 303, 5 x 1,269, 32 x 1,276, 16 x 4,116 and 32 x 16,141 pairs (the Whisk group's
shape) -- which between them take both bucket-slot scans, both sides of the `many` rule, four window widths, one and several
sort blocks per member and the large-bucket queue under shared bases (tests/test_dacc_members_model.py proves the claims and
reads the plans).  Every shape carries every family at once: uniform checks, one constant over the whole CRS per member,
few values, the special scalars of the split, a member whose checks cancel, loose pairs with one at infinity; one point P
sits on 64 CRS slots of the all-equal segment, -P on 32, and three instance points are (0, 0) -- curdle_dacc_begin takes
them, so infinity is not kept to the loose pair.  Per case run_case of tests/test_dacc_members_gpu.py (rows, per-member sums,
the whole, no export, counters), then the profile of one more run: the entries are exactly the non-zero signed digits of the
model's scalars (zero scalars never become bucket entries) and the large-bucket queue ran where the claims say so, and did
not for a uniform-only control.  Then the last accepted shape, four accumulations beside an MSM, and the sensitivity of the
expected side."""
import threading

import numpy as np
import pytest

import dacc_members_model as MM
import dacc_model as M
from dacc_model import R
from test_dacc_members_gpu import run_case

pytestmark = pytest.mark.gpu

NAMES = [s[0] for s in MM.MID_SHAPES]


@pytest.fixture(scope="module")
def base_pts(gpu):
    return gpu.Rand(2024).get_g1_affines(257)


@pytest.fixture(scope="module")
def mid(gpu, oracle, base_pts):
    """name -> (case, check_member, extra_member, claims, points, the packed arguments of dacc_run_members), made once."""
    out = {}
    cases = dict(MM.mid_cases(), **{"uniform-control": MM.uniform_control()})
    for name, (c, cmem, xmem, cl) in cases.items():
        pts = MM.mid_points(c, cl, base_pts, oracle)
        packed = (pts[1], M.pack_checks(c.checks), cmem, cl["shape"][3], M.pack_fr(c.pool, oracle), pts[2],
                  M.pack_fr(c.extra_scalars, oracle), xmem)
        out[name] = (c, cmem, xmem, cl, pts, packed)
    return out


@pytest.fixture(scope="module")
def resident(gpu, mid):
    sets = {}

    def get(name):
        if name not in sets:
            sets[name] = gpu.DBases(mid[name][4][0].copy())
        return sets[name]
    yield get
    for b in sets.values():
        b.free()


def profiled_run(gpu, bases, packed):
    """One more member-form run under the phase profile: (sums, profile)."""
    gpu.profile_enable(1)
    try:
        out, _ = gpu.dacc_run_members(bases, *packed, export=False)
        prof = gpu.profile_last()
    finally:
        gpu.profile_enable(0)
    return out, prof


def check_profile(gpu, name, c, cmem, xmem, cl, bases, packed):
    k = cl["shape"][3]
    plain, _ = gpu.dacc_run_members(bases, *packed, export=False)
    out, prof = profiled_run(gpu, bases, packed)
    rows = MM.member_rows(c.checks, cmem, k, c.pool, c.n_crs, c.n_inst)
    loose = MM.member_loose(c.extra_scalars, xmem, k)
    want = MM.model_entries(rows, loose, prof["window_bits"])
    nonzero = sum(1 for r, lo in zip(rows, loose) for v in list(r) + list(lo) if v)
    print(f"{name}: c={prof['window_bits']} windows={prof['num_windows']} entries={prof['entries']} (model {want}, "
          f"{nonzero} non-zero scalars) fragments={prof['fragments']} large_buckets={prof['large_buckets']}")
    assert (out == plain).all(), (name, "the sums differ under the profile")
    assert prof["window_bits"] == cl["plan"]["c"] and prof["num_windows"] == len(MM.window_widths(cl["plan"]["c"])), (name, prof)
    assert prof["entries"] == want, (name, "the sorted entries are not the non-zero digits of the model's scalars", prof, want)
    assert prof["entries"] <= nonzero * 2 * prof["num_windows"], (name, prof)
    return prof


@pytest.mark.parametrize("name", NAMES)
def test_mid_case_matches_the_model_and_the_oracle(gpu, oracle, coracle, base_pts, mid, resident, name):
    c, cmem, xmem, cl, pts, packed = mid[name]
    k = cl["shape"][3]
    run_case(gpu, oracle, coracle, base_pts, resident(name), c, cmem, xmem, k, points=pts)
    # (run_case has compared the empty members and the cancelling member's sum with the oracle's MSM of a zero row; here: its encoding)
    out, rows = gpu.dacc_run_members(resident(name), *packed)
    inf = coracle.msm_pippenger(pts[0][:1], np.zeros((1, 4), dtype=np.uint64))
    for j in cl["empty"] + (cl["cancelling"],):
        assert (out[j] == inf).all() and not rows[j].any(), (name, j, "not the oracle's infinity")
    assert cmem.count(cl["cancelling"]) == 2
    prof = check_profile(gpu, name, c, cmem, xmem, cl, resident(name), packed)
    assert cl["large"] == (c.n_res >= 1100)
    if cl["large"]:
        assert prof["large_buckets"] > 0, (name, "the large-bucket queue did not run", prof)
    assert gpu.msm_free_slots() == gpu.MSM_SLOTS


def test_uniform_control_stays_out_of_the_large_bucket_queue(gpu, oracle, coracle, base_pts, mid, resident):
    """The many-1100-168 shape rebuilt from the uniform family alone (segments of at most 8 slots: uniform_control's
    docstring has the bound): the same plan, the same checks of the sums, and not one bucket in the queue."""
    name = "uniform-control"
    c, cmem, xmem, cl, pts, packed = mid[name]
    run_case(gpu, oracle, coracle, base_pts, resident(name), c, cmem, xmem, cl["shape"][3], points=pts)
    prof = check_profile(gpu, name, c, cmem, xmem, cl, resident(name), packed)
    assert prof["large_buckets"] == 0 and prof["entries"] > 0, prof


def test_rows_of_zeros_leave_no_entry(gpu, oracle, coracle, base_pts, mid, resident):
    """Three members over the two-300 shape whose rows are all zero -- two of them hold that case's cancelling pair, one
    has nothing -- and no loose pair: every sum is infinity and the sort holds no entry at all."""
    c, cmem, xmem, cl, pts, packed = mid["two-300"]
    pair = [ck for ck, m in zip(c.checks, cmem) if m == cl["cancelling"]]
    assert len(pair) == 2 and not any(M.slots(pair, c.pool, c.n_crs, c.n_inst))
    none12, none4 = np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)
    args = (pts[1], M.pack_checks(pair + pair), [0, 0, 2, 2], 3, packed[4], none12, none4, [])
    out, rows = gpu.dacc_run_members(resident("two-300"), *args)
    inf = coracle.msm_pippenger(pts[0][:1], np.zeros((1, 4), dtype=np.uint64))
    assert (out == inf).all() and not rows.any()
    out, prof = profiled_run(gpu, resident("two-300"), args)
    print("rows of zeros:", prof)
    assert (out == inf).all() and prof["entries"] == 0 and prof["large_buckets"] == 0, prof


def test_last_accepted_shape(gpu, oracle, coracle, base_pts):
    """64 members x 65,535 CRS points, no instance points: k * NB = 64 x 36,864 = 2,359,296 bucket slots of the 4,194,304
    that one pass holds (kMaxSlotsPerPass); one more base gives c = 15, 64 x 90,112 slots, and is refused
    (tests/test_dacc_members_gpu.py).  Only members 1, 31, 32 and 62 carry checks -- a constant over the whole CRS each,
    65,535 equal scalars -- so the model's side is four rows and four oracle MSMs, while the kernels recode, scan and reduce
    all 64 members' slots.  (CPU side: four members live by the issue's design; nothing was cut.)"""
    c, cmem, xmem, cl = MM.last_accepted_case()
    k = MM.LAST_ACCEPTED["n_members"]
    crs, inst, loose = MM.mid_points(c, cl, base_pts, oracle)
    bases = gpu.DBases(crs.copy())
    try:
        args = (inst, M.pack_checks(c.checks), cmem, k, M.pack_fr(c.pool, oracle), loose, np.zeros((0, 4), dtype=np.uint64), xmem)
        before = gpu.stat_dacc_members()
        out, rows = gpu.dacc_run_members(bases, *args)
        after = gpu.stat_dacc_members()
        assert after == dict(before, runs=before["runs"] + 1, members=before["members"] + k), (before, after)
        assert out.shape == (k, 18) and rows.shape == (k, c.n_crs, 4)
        inf = coracle.msm_pippenger(crs[:1], np.zeros((1, 4), dtype=np.uint64))
        want = {j: M.slots(MM.member_checks(c.checks, cmem, j), c.pool, c.n_crs, 0) for j in cl["carriers"]}
        n_inf = 0
        for j in range(k):
            if j in want:
                raw = M.raw_ints(rows[j])
                assert all(v < R for v in raw), (j, "an exported element is not canonical")
                assert [v * oracle.R_FR_INV % R for v in raw] == want[j], (j, "slot scalars differ from the model")
                exp = coracle.msm_pippenger(crs, M.pack_fr(want[j], oracle), threads=4)
                assert (out[j] == exp).all() and not (exp == inf).all(), (j, "the sum differs from the oracle's MSM of its map")
            else:
                n_inf += 1
                assert not rows[j].any() and (out[j] == inf).all(), (j, "a member without checks is not infinity")
        assert n_inf == 60
        whole, _ = gpu.dacc_run(bases, *(args[:2] + args[4:7]), export=False)
        assert (coracle.jac_normalise(gpu.g1_sum(out)) == coracle.jac_normalise(whole)).all(), "the members' sums do not add up"
        out2, prof = profiled_run(gpu, bases, args)
        print(f"last-accepted: c={prof['window_bits']} windows={prof['num_windows']} entries={prof['entries']} "
              f"fragments={prof['fragments']} large_buckets={prof['large_buckets']}")
        assert (out2 == out).all() and prof["large_buckets"] > 0
        loose_sc = [[]] * 4
        assert prof["entries"] == MM.model_entries([want[j] for j in cl["carriers"]], loose_sc, prof["window_bits"]), prof
        assert gpu.msm_free_slots() == gpu.MSM_SLOTS
    finally:
        bases.free()


def test_four_accumulations_beside_an_msm(gpu, oracle, coracle, mid, resident):
    """Four threads, each with a different mid case on an accumulation of its own, and a fifth with curdle_msm_g1 over
    40,000 pairs: every result is the sequential one, and every workspace slot comes back."""
    names = NAMES[:4]
    kq = oracle.Rand(40).get_frs(2)
    pts = coracle.points_walk(kq[0], kq[1], 40000)
    rng = np.random.default_rng(40)
    sc = rng.integers(0, 1 << 64, size=(40000, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    bases = {n: resident(n) for n in names}
    seq = {n: gpu.dacc_run_members(bases[n], *mid[n][5], export=False)[0] for n in names}
    seq["msm"] = gpu.msm_g1(pts, sc)
    assert (seq["msm"] == coracle.msm_pippenger(pts, sc, threads=4)).all()
    got, errors = {}, []
    start = threading.Barrier(5)

    def work(n):
        try:
            start.wait()
            got[n] = gpu.msm_g1(pts, sc) if n == "msm" else gpu.dacc_run_members(bases[n], *mid[n][5], export=False)[0]
        except Exception as e:      # noqa: BLE001 -- reported below, in the test's thread
            errors.append((n, repr(e)))

    threads = [threading.Thread(target=work, args=(n,)) for n in names + ["msm"]]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for n in names + ["msm"]:
        assert (got[n] == seq[n]).all(), (n, "differs from the sequential result")
    assert gpu.msm_free_slots() == gpu.MSM_SLOTS


@pytest.mark.parametrize("what", ("a check moved to the neighbouring member", "a loose pair dropped", "a zero of the cancelling row set to 1"))
def test_run_case_notices_a_wrong_expected_side(gpu, oracle, coracle, base_pts, mid, resident, monkeypatch, what):
    """The checks of run_case are sensitive: each of three changes of the MODEL's side alone makes it fail (the library's
    inputs stay as they are; no kernel is changed)."""
    name = "five-264-1000"
    c, cmem, xmem, cl, pts, packed = mid[name]
    k = cl["shape"][3]
    rows_of, loose_of = MM.member_rows, MM.member_loose
    if what.startswith("a check"):
        i = next(i for i, ck in enumerate(c.checks) if any(M.slots([ck], c.pool, c.n_crs, c.n_inst)))
        moved = list(cmem)
        moved[i] = (moved[i] + 1) % k
        monkeypatch.setattr(MM, "member_rows", lambda checks, cm_, *a: rows_of(checks, moved, *a))
        expect = "slot scalars differ from the model"
    elif what.startswith("a loose"):
        e = next(e for e, s in enumerate(c.extra_scalars) if s and pts[2][e].any())

        def dropped(xs, xm, n):
            return loose_of([0 if i == e else s for i, s in enumerate(xs)], xm, n)
        monkeypatch.setattr(MM, "member_loose", dropped)
        expect = "the sum differs from the oracle's MSM"
    else:
        def one(*a):
            rows = rows_of(*a)
            z = rows[cl["cancelling"]]
            assert not any(z)
            z[MM.P_SLOTS[0]] = 1
            return rows
        monkeypatch.setattr(MM, "member_rows", one)
        expect = "slot scalars differ from the model"
    with pytest.raises(AssertionError, match=expect):
        run_case(gpu, oracle, coracle, base_pts, resident(name), c, cmem, xmem, k, points=pts)
    monkeypatch.undo()
    run_case(gpu, oracle, coracle, base_pts, resident(name), c, cmem, xmem, k, points=pts)      # ... and passes untouched
    assert gpu.msm_free_slots() == gpu.MSM_SLOTS
