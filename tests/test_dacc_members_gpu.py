"""curdle_dacc_run_members on the GPU against the member model (tests/dacc_members_model.py) and the C oracle, bit for
bit: 1, 2, 5, 32 and 64 members over n_crs = 20 with n_inst = 16 and with n_inst = 0 -- empty first, middle and last
members, two members on the same slots, loose pairs spread over the members with one at infinity -- and two members
beyond 16,384 bases (dacc_model's `routes` shape, where a single accumulation takes the separate scalar build).  Per case:
the exported rows == the model's rows; every member's sum == the oracle's MSM of that member's (base, scalar) map; the sum
of the members' sums == curdle_dacc_run on the whole description; one member == curdle_dacc_run bit for bit.  Then the
refusals, which must leave the counters and the workspace slots as they were."""
import numpy as np
import pytest

import dacc_members_model as MM
import dacc_model as M
from dacc_model import R

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 5, 32, 64)


@pytest.fixture(scope="module")
def base_pts(gpu):
    return gpu.Rand(2024).get_g1_affines(257)


@pytest.fixture(scope="module")
def resident(gpu, base_pts):
    sets = {}

    def get(n_crs):
        if n_crs not in sets:
            sets[n_crs] = gpu.DBases(base_pts[np.arange(n_crs) % len(base_pts)].copy())
        return sets[n_crs]
    yield get
    for b in sets.values():
        b.free()


def run_case(gpu, oracle, coracle, base_pts, bases, c, cmem, xmem, n_members, points=None):
    """`points`: the case's (crs, inst, loose) where they are not case_points' tiling (tests/test_dacc_members_mid_gpu.py)."""
    crs, inst, loose = points or M.case_points(c, base_pts)
    args = (inst, M.pack_checks(c.checks), M.pack_fr(c.pool, oracle), loose, M.pack_fr(c.extra_scalars, oracle))
    before = gpu.stat_dacc_members()
    out, rows = gpu.dacc_run_members(bases, args[0], args[1], cmem, n_members, args[2], args[3], args[4], xmem)
    after = gpu.stat_dacc_members()
    assert after == dict(before, runs=before["runs"] + 1, members=before["members"] + n_members), (c.name, before, after)
    want = MM.member_rows(c.checks, cmem, n_members, c.pool, c.n_crs, c.n_inst)
    loose_sc = MM.member_loose(c.extra_scalars, xmem, n_members)
    pts = np.concatenate([crs, inst, loose])
    assert out.shape == (n_members, 18) and rows.shape == (n_members, c.n_res, 4)
    for j in range(n_members):
        raw = M.raw_ints(rows[j])                                                     # 1. the rows, canonical and equal
        assert all(v < R for v in raw), (c.name, j, "an exported element is not canonical")
        got = [v * oracle.R_FR_INV % R for v in raw]
        assert got == want[j], (c.name, f"member {j}: slot scalars differ from the model, first at "
                                f"{[i for i in range(c.n_res) if got[i] != want[j][i]][:1]}")
        exp = coracle.msm_pippenger(pts, M.pack_fr(want[j] + loose_sc[j], oracle), threads=4)
        assert (out[j] == exp).all(), (c.name, f"member {j}: the sum differs from the oracle's MSM of its map")   # 2.
        if j not in cmem and j not in xmem:
            assert not any(want[j]) and (out[j] == coracle.msm_pippenger(pts[:1], np.zeros((1, 4), dtype=np.uint64))).all(), \
                (c.name, j, "a member without checks and loose pairs is not infinity")
    whole, whole_sc = gpu.dacc_run(bases, *args)
    total = gpu.g1_sum(out)                                                            # 3. the members add up to the group
    assert (coracle.jac_normalise(total) == coracle.jac_normalise(whole)).all(), (c.name, "the members' sums do not add up")
    if n_members == 1:                                                                 # 4. one member: the same bits
        assert (out[0] == whole).all() and (rows[0] == whole_sc).all(), c.name
    out2, none = gpu.dacc_run_members(bases, args[0], args[1], cmem, n_members, args[2], args[3], args[4], xmem, export=False)
    assert none is None and (out2 == out).all(), (c.name, "the sums differ without export_scalars")
    return args


@pytest.mark.parametrize("n_inst", (16, 0))
@pytest.mark.parametrize("n_members", COUNTS)
def test_members_match_the_model_and_the_oracle(gpu, oracle, coracle, base_pts, resident, n_members, n_inst):
    c, cmem, xmem = MM.group_case(20, n_inst, n_members, 1)
    assert M.validate(c.checks, len(c.pool), c.n_crs, c.n_inst, c.n_extra) and MM.validate_members(cmem, xmem, n_members)
    if n_members >= 5:
        assert all(j not in cmem and j not in xmem for j in (0, n_members // 2, n_members - 1))
    if n_members >= 2:
        assert cmem[-1] != cmem[-2]                     # the checks on the same slots belong to two members
    run_case(gpu, oracle, coracle, base_pts, resident(20), c, cmem, xmem, n_members)


def test_two_members_beyond_16384_bases(gpu, oracle, coracle, base_pts, resident):
    c = [c for c in M.family("routes") if M.path(c.n_total, len(c.pool), len(c.checks)) == "split_lds"][0]
    assert c.n_total > M.FUSED_MAX and c.inf_extra >= 0
    cmem = [0, 1, 0, 1]
    xmem = [e % 2 for e in range(c.n_extra)]
    run_case(gpu, oracle, coracle, base_pts, resident(c.n_crs), c, cmem, xmem, 2)


def test_no_members_and_nothing_to_sum(gpu, oracle, resident):
    before = gpu.stat_dacc_members()
    out, rows = gpu.dacc_run_members(resident(20), np.zeros((0, 12), dtype=np.uint64), M.pack_checks([]), [], 0,
                                     np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 12), dtype=np.uint64),
                                     np.zeros((0, 4), dtype=np.uint64), [])
    assert out.shape == (0, 18) and gpu.msm_free_slots() == gpu.MSM_SLOTS and gpu.stat_dacc_members() == before


def test_refusals_launch_nothing_and_keep_no_slot(gpu, oracle, base_pts, resident):
    c, cmem, xmem = MM.group_case(20, 16, 5, 1)
    _, inst, loose = M.case_points(c, base_pts)
    checks, pool, xs = M.pack_checks(c.checks), M.pack_fr(c.pool, oracle), M.pack_fr(c.extra_scalars, oracle)
    assert gpu.msm_free_slots() == gpu.MSM_SLOTS
    before = gpu.stat_dacc_members()

    def refused(what, bases=None, inst=inst, checks=checks, cmem=cmem, n_members=5, pool=pool, loose=loose, xs=xs, xmem=xmem):
        with pytest.raises(gpu.CurdleError) as e:
            gpu.dacc_run_members(bases or resident(20), inst, checks, cmem, n_members, pool, loose, xs, xmem, check_members=False)
        assert e.value.code == gpu.EINVAL, (what, e.value)
        assert gpu.stat_dacc_members() == before, what
        assert gpu.msm_free_slots() == gpu.MSM_SLOTS, what

    refused("a check's member == n_members", cmem=[5] + cmem[1:])
    refused("a check's member far outside", cmem=cmem[:-1] + [0xFFFFFFFF])
    refused("a loose pair's member == n_members", xmem=xmem[:-1] + [5])
    refused("checks and loose pairs without a member", n_members=0)
    none = np.zeros((0, 12), dtype=np.uint64)
    refused("loose pairs without a member", n_members=0, checks=M.pack_checks([]), cmem=[])
    refused("checks without a member", n_members=0, loose=none, xs=np.zeros((0, 4), dtype=np.uint64), xmem=[])
    refused("more members than CURDLE_DACC_MAX_MEMBERS", n_members=MM.MAX_MEMBERS + 1)
    # what curdle_dacc_run refuses: an unknown kind, a segment past its set, an offset outside the pool
    for what, field, value in (("kind", 0, 4), ("segment", 13, 17), ("pool", 4, len(c.pool))):
        bad = checks.copy()
        row = next(i for i in range(len(bad)) if bad[i, 10])          # a check with a segment
        bad[row, field] = value
        assert not M.validate([M.Check(*[int(v) for v in bad[row, :10]], tuple(M.Seg(*[int(v) for v in bad[row, 11 + 4 * s:15 + 4 * s]])
                                                                         for s in range(int(bad[row, 10]))))],
                              len(c.pool), c.n_crs, c.n_inst, c.n_extra), what
        refused(f"a malformed check ({what})", checks=bad)
    # the form's limits: 64 members x 65,537 resident slots; 64 x 65,536 fit that limit and not one pass of bucket slots
    big = gpu.DBases(base_pts[np.arange(65536) % len(base_pts)].copy())
    try:
        zero4 = np.zeros((0, 4), dtype=np.uint64)
        on_crs = M.pack_checks([k._replace(segs=tuple(s._replace(set=M.SET_CRS) for s in k.segs)) for k in c.checks[-4:]])
        kw = dict(bases=big, checks=on_crs, cmem=[0, 63, 0, 63], n_members=64, loose=none, xs=zero4, xmem=[])
        refused("members x slots beyond CURDLE_DACC_MAX_MEMBER_SLOTS", inst=inst[:1], **kw)
        refused("more bucket slots than one pass holds", inst=none, **kw)
    finally:
        big.free()
    # ... and the accumulator still runs
    out, _ = gpu.dacc_run_members(resident(20), inst, checks, cmem, 5, pool, loose, xs, xmem)
    assert out.shape == (5, 18) and gpu.msm_free_slots() == gpu.MSM_SLOTS
