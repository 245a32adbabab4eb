"""The member model (tests/dacc_members_model.py) against dacc_model: the rows of the members add up to the slots of
the whole description, a member without checks has a zero row, and the rule for member indices.  No GPU."""
import numpy as np
import pytest

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
