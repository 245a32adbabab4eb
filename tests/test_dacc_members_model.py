"""The member model (tests/dacc_members_model.py) against dacc_model: the rows of the members add up to the slots of
the whole description, a member without checks has a zero row, and the rule for member indices.  Then the mid-size cases
(mid_cases): what the generator claims, proved per case, and the plan paths every shape is there for, read from the host-only
plan probe (tests/plan_probe.cpp, `members`).  No GPU.

The sanitizer stand-in (`host_flow dacc`, tests/hostbuild/) has curdle_dacc_run and the two-step form only: it cannot take
the member form, so no mid case runs through it."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

import dacc_members_model as MM
import dacc_model as M
from dacc_model import R

FAMS = ("random", "overlap", "special")
COUNTS = (1, 2, 5, 32)


@pytest.mark.parametrize("fam", FAMS)
def test_member_rows_sum_to_the_slots_of_all_checks(fam):
    rng = np.random.default_rng([9, FAMS.index(fam)])
    cases = M.family(fam)
    for i, c in enumerate(cases[::3] if fam == "random" else cases):
        whole = M.slots(c.checks, c.pool, c.n_crs, c.n_inst)
        for n_members in COUNTS:
            hole = MM.empties(n_members)
            cmem = MM.assign(rng, len(c.checks), n_members, hole)
            assert MM.validate_members(cmem, [], n_members)
            rows = MM.member_rows(c.checks, cmem, n_members, c.pool, c.n_crs, c.n_inst)
            assert len(rows) == n_members and all(len(r) == c.n_res for r in rows)
            for s in range(c.n_res):
                assert sum(r[s] for r in rows) % R == whole[s], (c.name, n_members, s)
            for j in range(n_members):
                if j not in cmem:
                    assert not any(rows[j]), (c.name, n_members, j, "a member without checks has a non-zero row")
            for j in hole:
                assert j not in cmem


def test_one_member_is_the_whole_description():
    for c in M.family("overlap"):
        assert MM.member_rows(c.checks, [0] * len(c.checks), 1, c.pool, c.n_crs, c.n_inst) == [M.slots(c.checks, c.pool, c.n_crs, c.n_inst)]


def test_overlapping_members_keep_their_rows_apart():
    """Two members on the same slots: each row holds its own member's elements there, not the sum."""
    for n_inst in (16, 0):
        c, cmem, xmem = MM.group_case(20, n_inst, 2, 1)
        rows = MM.member_rows(c.checks, cmem, 2, c.pool, c.n_crs, c.n_inst)
        at = (20 if n_inst else 0) + 3
        assert rows[0][at] and rows[1][at] and rows[0][at] != rows[1][at]
        assert (rows[0][at] + rows[1][at]) % R == M.slots(c.checks, c.pool, c.n_crs, c.n_inst)[at]
        assert M.validate(c.checks, len(c.pool), c.n_crs, c.n_inst, c.n_extra) and MM.validate_members(cmem, xmem, 2)


def test_group_cases_leave_the_promised_members_empty():
    for n_members in (5, 32, 64):
        c, cmem, xmem = MM.group_case(20, 16, n_members, 1)
        for j in MM.empties(n_members):
            assert j not in cmem and j not in xmem
        assert len(cmem) == len(c.checks) and len(xmem) == c.n_extra == 5 and c.inf_extra == 1
        loose = MM.member_loose(c.extra_scalars, xmem, n_members)
        assert [sum(col) % R for col in zip(*loose)] == [s % R for s in c.extra_scalars]


def test_member_index_rule():
    assert MM.validate_members([], [], 0)
    assert not MM.validate_members([0], [], 0) and not MM.validate_members([], [0], 0)
    assert MM.validate_members([0, 4], [4], 5)
    assert not MM.validate_members([5], [], 5) and not MM.validate_members([], [5], 5)
    assert not MM.validate_members([1 << 32 - 1], [], 64)
    assert MM.validate_members([], [], 3)                      # members without anything are fine


# --------------------------------------------------------------------------- the mid-size cases ---
@pytest.fixture(scope="module")
def mid():
    return MM.mid_cases()


@pytest.fixture(scope="module")
def probe(cm, tmp_path_factory):
    """plan_probe members n_tot k -> the plan's fields and the windows' widths."""
    exe = str(tmp_path_factory.mktemp("plan") / "plan_probe")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "plan_probe.cpp"), "-L" + PKG, "-lcurdlemsm", "-Wl,-rpath," + PKG,
                           "-o", exe])

    def members(n_tot, k):
        out = subprocess.run([exe, "members", str(n_tot), str(k)], capture_output=True, text=True).stdout.splitlines()
        head, *kv = out[0].split()
        assert head == "members"
        row = {a: int(b) for a, b in (x.split("=") for x in kv)}
        if row["rc"] == 0:
            row["widths"] = [int(x.split(":")[0]) for x in out[1].split()[1:]]
        return row
    return members


def test_mid_cases_are_valid_and_hold_what_they_claim(mid):
    assert list(mid) == [s[0] for s in MM.MID_SHAPES] and MM.mid_cases() == mid                 # the same on every call
    for name, (c, cmem, xmem, cl) in mid.items():
        n_crs, n_inst, n_extra, k = cl["shape"]
        assert (c.n_crs, c.n_inst, c.n_extra) == (n_crs, n_inst, n_extra) and cl["families"] == MM.FAMILY_NAMES, name
        assert M.validate(c.checks, len(c.pool), n_crs, n_inst, n_extra) and MM.validate_members(cmem, xmem, k), name
        assert len(cmem) == len(c.checks) and len(xmem) == n_extra == len(c.extra_scalars), name
        rows = MM.member_rows(c.checks, cmem, k, c.pool, n_crs, n_inst)
        # the first, a middle and the last member have nothing
        assert cl["empty"] == MM.empties(k), name
        for j in cl["empty"]:
            assert j not in cmem and j not in xmem and not any(rows[j]), (name, j)
        # the cancelling member: checks, no loose pair, and a row of zeros
        z = cl["cancelling"]
        assert cmem.count(z) == 2 and z not in xmem and not any(rows[z]), name
        assert all(any(M.slots([ck], c.pool, n_crs, n_inst)) for ck in MM.member_checks(c.checks, cmem, z)), name
        # all-equal: [0, N_EQ) of the CRS holds one value per worker, another one for every worker
        consts = cl["all_equal"]
        assert set(consts) == set(cl["workers"]) and len(set(consts.values())) == len(consts), name
        for j, v in consts.items():
            assert v and rows[j][:MM.N_EQ] == [v] * MM.N_EQ, (name, j)
        assert max(MM.P_SLOTS + MM.NEG_SLOTS) < MM.N_EQ and len(MM.P_SLOTS) >= 64 and len(MM.NEG_SLOTS) == 32
        assert not set(MM.P_SLOTS) & set(MM.NEG_SLOTS)
        # ... and one worker holds a constant over a whole instance range, where there are instance points
        w0 = cl["workers"][0]
        assert MM.glv_split(consts[w0])[0] == MM.glv_split(consts[w0])[1] > 0, name              # equal halves: one bucket per window
        if n_inst:
            j, lo, ln = cl["inst_const"]
            assert j == w0 and ln >= 168 and all(lo <= s < lo + ln for s in cl["inf_inst"]) and len(cl["inf_inst"]) == 3, name
            if cl["exact_roles"]:
                assert rows[j][n_crs + lo:n_crs + lo + ln] == [consts[j]] * ln and rows[j][:n_crs] == [consts[j]] * n_crs, name
            assert all(rows[j][n_crs + s] for s in cl["inf_inst"]), name                          # infinity with a scalar that is not zero
        # few values: w q, -w q^2, w q^3 and +-w q^4 over at least 1,024 slots where the shape has that many beside the all-equal segment
        j, n, q_cap = cl["few_values"]
        ck = [x for x in MM.member_checks(c.checks, cmem, j) if x.kind == M.FOLD_POW and x.q_cap == q_cap and x.n_struct == n]
        assert len(ck) == 1 and len(set(M.vector(ck[0], c.pool))) == q_cap + 2 and sum(s.len for s in ck[0].segs) == n, name
        assert n >= 1024 or n_crs - MM.N_EQ + (MM.WHISK_RANGE if name.startswith("whisk") else n_inst) < 1024, name
        # specials: every value of the list in the pool, multiplied by alpha = 1; exactly the slot's scalar where the roles are apart
        j, st, first, ln = cl["specials"]
        vals = MM.special_values()
        ck = [x for x in MM.member_checks(c.checks, cmem, j) if x.kind == M.EXPLICIT and x.n_tail == ln == len(vals)]
        assert ck and c.pool[ck[-1].tail_off:ck[-1].tail_off + ln] == vals and c.pool[ck[-1].alpha_off] == 1, name
        assert set(M.SPECIALS.values()) <= set(vals) and len(vals) > 50
        if cl["exact_roles"] and n_inst:
            assert st == M.SET_INST and rows[j][n_crs + first:n_crs + first + ln] == vals, name
        # loose pairs: on workers only, one at infinity, special scalars among them (0 too from four pairs on)
        assert set(xmem) <= set(cl["workers"]) and c.inf_extra == 1 and c.extra_scalars[0] == R - 1, name
        assert len(set(xmem)) == min(n_extra, len(cl["workers"])), name
        # the Whisk group's shape: member j names the CRS and its own 496 instance slots
        if name.startswith("whisk"):
            assert n_inst == k * MM.WHISK_RANGE
            for j in range(k):
                own = range(n_crs + MM.WHISK_RANGE * j, n_crs + MM.WHISK_RANGE * (j + 1))
                assert all(s in own for s in range(n_crs, n_crs + n_inst) if rows[j][s]), (name, j)
            assert sum(any(rows[j][n_crs:]) for j in range(k)) >= len(cl["workers"]) // 2
        # the members' rows add up to the slots of all checks
        whole = M.slots(c.checks, c.pool, n_crs, n_inst)
        assert [sum(col) % R for col in zip(*rows)] == whole, name


def test_mid_points_repeat_a_point_negate_it_and_put_infinity_among_the_instance_points(mid, cm, oracle):
    base_pts = cm.Rand(2024).get_g1_affines(257)
    for name, (c, cmem, xmem, cl) in mid.items():
        crs, inst, loose = MM.mid_points(c, cl, base_pts, oracle)
        p = crs[MM.P_SLOTS[0]]
        assert p.any() and all((crs[s] == p).all() for s in MM.P_SLOTS), name
        neg = crs[MM.NEG_SLOTS[0]]
        assert (neg[:6] == p[:6]).all() and all((crs[s] == neg).all() for s in MM.NEG_SLOTS), name
        assert (oracle._from_limbs(neg[6:12]) + oracle._from_limbs(p[6:12])) % oracle.P == 0, name
        assert crs.any(axis=1).all(), name                                                      # the CRS stays finite
        assert sum(not r.any() for r in inst) == (3 if c.n_inst else 0) and not loose[1].any(), name
        assert loose.any(axis=1).sum() == c.n_extra - 1, name


def test_the_restated_split_and_window_widths_are_the_librarys(probe):
    import test_abi
    assert MM.GLV_LAMBDA == test_abi.GLV_LAMBDA
    rng = np.random.default_rng(5)
    for v in MM.special_values() + M._frs(rng, 200):
        k1, k2 = MM.glv_split(v)
        assert (k1, k2) == test_abi.glv_split(v, R) and (k1 + k2 * MM.GLV_LAMBDA - v) % R == 0
        assert abs(k1) < 1 << 127 and abs(k2) < 1 << 127
        for c in (9, 10, 11, 12, 14):                     # the digits are the halves again
            widths, at = MM.window_widths(c), 0
            assert sum(widths) == 127
            assert (MM.nonzero_digits(v, widths) == 0) == (v == 0)
    for name, n_crs, n_inst, n_extra, k, own, plan in MM.MID_SHAPES:
        got = probe(n_crs + n_inst + n_extra, k)
        assert got["widths"] == MM.window_widths(got["c"]), name
    # a digit by hand: 2^c - 1 in the lowest window is -1 and a carry
    assert MM.nonzero_digits((1 << 10) - 1, MM.window_widths(10)) == 2 and MM.nonzero_digits(1 << 9, MM.window_widths(10)) == 1


def test_every_mid_shape_reaches_the_plan_paths_it_claims(mid, probe):
    seen = []
    for name, (c, cmem, xmem, cl) in mid.items():
        n_crs, n_inst, n_extra, k = cl["shape"]
        got = probe(c.n_total, k)
        print(name, got)
        assert got["rc"] == 0 and got["fits"] == 1 and got["max_small"] == 16, (name, got)
        assert got["slots"] == k * got["NB"] and (got["fuse_scan"] == 2) == (got["slots"] <= 32768), (name, got)
        assert got["gpu_combine"] == (1 if k >= 12 else 0), (name, got)
        assert got["sort_blocks"] == -(-2 * c.n_total // got["chunk"]), (name, got)
        assert {f: got[f] for f in cl["plan"]} == cl["plan"], (name, got)
        seen.append(got)
        # the large-bucket queue: the worker whose halves are equal fills one bucket per window with two entries per slot
        # that holds its constant -- more than max_small fragments of L entries where the claim says so
        w0 = cl["workers"][0]
        row = MM.member_rows(c.checks, cmem, k, c.pool, n_crs, n_inst)[w0]
        run = 2 * row.count(cl["all_equal"][w0])
        assert (-(-run // got["L"]) > got["max_small"]) or not cl["large"], (name, run, got)
        assert cl["large"] == (n_crs + n_inst >= 1100), name
    assert {g["fuse_scan"] for g in seen} == {2, 3}                       # k_scan_one and k_scan_chain
    assert {g["gpu_combine"] for g in seen} == {0, 1}                     # both sides of the `many` rule
    assert len({g["c"] for g in seen}) >= 3
    assert min(g["sort_blocks"] for g in seen) == 1 and max(g["sort_blocks"] for g in seen) > 1
    assert any(g["sort_blocks"] > 1 and g["k"] > 2 for g in seen)         # several sort blocks per member, more than two members


def test_the_uniform_control_cannot_reach_the_large_bucket_queue(probe):
    c, cmem, xmem, cl = MM.uniform_control()
    n_crs, n_inst, n_extra, k = cl["shape"]
    assert M.validate(c.checks, len(c.pool), n_crs, n_inst, n_extra) and MM.validate_members(cmem, xmem, k)
    assert cl["families"] == ("uniform",) and cl["cancelling"] is None and not cl["all_equal"] and not cl["large"]
    got = probe(c.n_total, k)
    assert {f: got[f] for f in cl["plan"]} == cl["plan"]
    rows = MM.member_rows(c.checks, cmem, k, c.pool, n_crs, n_inst)
    assert sum(any(r) for r in rows) >= 20
    longest = max(max((r.count(v) for v in set(r) if v), default=0) for r in rows)
    assert 0 < longest <= 48                                              # six segments of eight slots
    assert -(-2 * longest // got["L"]) + 1 < got["max_small"]             # both halves in one bucket, cut by one more lane


def test_the_last_accepted_shape_is_the_last(probe):
    la = MM.LAST_ACCEPTED
    c, cmem, xmem, cl = MM.last_accepted_case()
    k = la["n_members"]
    assert k == MM.MAX_MEMBERS and (c.n_crs, c.n_inst, c.n_extra) == (la["n_crs"], 0, 0) and k * c.n_crs <= MM.MAX_MEMBER_SLOTS
    assert M.validate(c.checks, len(c.pool), c.n_crs, 0, 0) and MM.validate_members(cmem, xmem, k)
    assert cl["carriers"] == (1, 31, 32, 62) and set(cmem) == set(cl["carriers"])
    got, over = probe(c.n_crs, k), probe(c.n_crs + 1, k)
    assert got["rc"] == 0 and got["NB"] == la["NB"] and got["slots"] == k * la["NB"] <= la["limit"] and got["fits"] == 1
    assert over["rc"] == 0 and over["slots"] > la["limit"] and over["fits"] == 0
