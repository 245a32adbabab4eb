"""The member form of the device accumulator (curdle_dacc_run_members) as a thin layer over the big-integer
model of tests/dacc_model.py: a member's row of slot scalars is dacc_model.slots over that member's checks,
nothing else.  Also the rule for member indices, seeded member assignments, and the descriptions the member
tests share.  No GPU, no library."""
import numpy as np

import dacc_model as M
from dacc_model import R

MAX_MEMBERS = 64                 # CURDLE_DACC_MAX_MEMBERS
MAX_MEMBER_SLOTS = 1 << 22       # CURDLE_DACC_MAX_MEMBER_SLOTS


def validate_members(check_member, extra_member, n_members) -> bool:
    """The header's rule: every index below n_members; no checks or loose pairs without a member."""
    idx = list(check_member) + list(extra_member)
    if n_members == 0:
        return not idx
    return all(0 <= m < n_members for m in idx)


def member_checks(checks, check_member, j) -> list:
    return [ck for ck, m in zip(checks, check_member) if m == j]


def member_rows(checks, check_member, n_members, pool, n_crs, n_inst) -> list:
    """rows[j] = slots(member j's checks)."""
    return [M.slots(member_checks(checks, check_member, j), pool, n_crs, n_inst) for j in range(n_members)]


def member_loose(extra_scalars, extra_member, n_members) -> list:
    """loose[j][e] = the scalar of loose pair e in member j's sum: its own, or 0."""
    return [[s if m == j else 0 for s, m in zip(extra_scalars, extra_member)] for j in range(n_members)]


def assign(rng, n, n_members, empty=()) -> list:
    """n seeded member indices below n_members, none of them in `empty`."""
    allowed = [j for j in range(n_members) if j not in set(empty)]
    return [allowed[int(rng.integers(len(allowed)))] for _ in range(n)] if allowed else []


def empties(n_members) -> tuple:
    """Members left without checks and loose pairs: the first, a middle one and the last, from five members on."""
    return (0, n_members // 2, n_members - 1) if n_members >= 5 else ()


def group_case(n_crs, n_inst, n_members, seed):
    """One description over (n_crs, n_inst) for n_members members: random valid checks (dacc_model's generator), two
    pairs of checks of different kinds that lie on the SAME slots and go to two different members, and five loose pairs,
    one of them at infinity.  Returns (case, check_member, extra_member)."""
    rng = np.random.default_rng([seed, n_crs, n_inst, n_members])
    b = M._Builder(rng)
    M._mixed_checks(b, rng, n_crs, n_inst, 10, max_len=16)
    n_mixed = len(b.checks)
    st, set_n = (M.SET_INST, n_inst) if n_inst else (M.SET_CRS, n_crs)
    for kind in (M.FOLD_POW, M.EXPLICIT, M.CONST, M.FOLD):          # all four on slots [3, 13) of one set
        b.check(kind, 0 if kind == M.EXPLICIT else 12, gammas=M._frs(rng, 4), tail=M._frs(rng, 12), q_cap=5,
                segs=[(st, 3, min(10, set_n - 3), 1)])
    case = b.case(n_crs, n_inst, 5, f"{n_members} members over ({n_crs}, {n_inst})", f"members-{n_crs}-{n_inst}-{n_members}",
                  inf_extra=1)
    hole = empties(n_members)
    check_member = assign(rng, n_mixed, n_members, hole)
    live = [j for j in range(n_members) if j not in hole]
    check_member += [live[0], live[-1], live[0], live[-1]]           # the overlapping checks: two members (one if there is one)
    extra_member = assign(rng, 5, n_members, hole)
    extra_member[1] = live[-1]                                       # the loose point at infinity has a member too
    return case, check_member, extra_member
