"""The member form of the device accumulator (curdle_dacc_run_members) as a thin layer over the big-integer
model of tests/dacc_model.py: a member's row of slot scalars is dacc_model.slots over that member's checks,
nothing else.  Also the rule for member indices, seeded member assignments, and the descriptions the member
tests share.  Then the mid-size cases (mid_cases, uniform_control, last_accepted_case): shapes chosen for the plan paths of
the batched MSM behind the member form, every family of rows at once, with a dict of claims per case that the CPU tests
prove and the GPU tests rely on; and a model of the sort's entry count (the non-zero signed digits of the split halves).
No GPU, no library."""
from collections import Counter

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


# ------------------------------------------------------------------------ mid-size member cases ---
GLV_LAMBDA = 0xac45a4010001a40200000000ffffffff      # z^2 - 1 (tests/test_abi.py): lambda^2 + lambda + 1 = r
N_EQ = 160          # CRS slots [0, N_EQ): named by nothing but the all-equal CONST checks (and the cancelling pair)
P_SLOTS = tuple(range(8, 136, 2))      # 64 CRS slots that hold one point P (mid_points)
NEG_SLOTS = tuple(range(9, 135, 4))    # 32 CRS slots that hold -P
WHISK_RANGE = 496   # instance slots of one member of the Whisk group's shape (ell = 124: 4 ell)

# (name, n_crs, n_inst, n_extra, members, own instance range per member, plan paths the shape is there for)
# The paths are what `plan_probe members n_crs+n_inst+n_extra members` prints (tests/test_dacc_members_model.py asserts it):
# c, fuse_scan (2: k_scan_one, 3: k_scan_chain), gpu_combine (the `many` rule), sort_blocks = ceil(2 n_tot / chunk).
# No shape had to be moved: 5 members are below gpu_combine_min() = 12, and 5 x 6,144 bucket slots still fit k_scan_one.
MID_SHAPES = (
    ("two-300", 300, 0, 3, 2, False, dict(c=10, fuse_scan=2, gpu_combine=0, sort_blocks=1)),
    ("five-264-1000", 264, 1000, 5, 5, False, dict(c=10, fuse_scan=2, gpu_combine=0, sort_blocks=1)),
    ("many-1100-168", 1100, 168, 8, 32, False, dict(c=9, fuse_scan=3, gpu_combine=1, sort_blocks=1)),
    ("blocks-2100-2000", 2100, 2000, 16, 16, False, dict(c=11, fuse_scan=3, gpu_combine=1, sort_blocks=3)),
    ("whisk-264-15872", 264, 15872, 5, 32, True, dict(c=12, fuse_scan=3, gpu_combine=1, sort_blocks=2)),
)
LAST_ACCEPTED = dict(n_crs=65535, n_members=64, NB=36864, limit=1024 * 4096)      # kMaxSlotsPerPass; 65,536 bases: NB = 90,112


def glv_boundaries() -> list:
    """The scalars where the branches of the split flip: the list of test_scalars_at_the_boundaries_of_the_split
    (tests/test_msm_gpu.py), restated."""
    lam, half = GLV_LAMBDA, (R - 1) // 2
    vals = [half + 1, half - 1, lam, lam - 1, lam + 1, lam >> 1, (lam >> 1) + 1, (lam >> 1) - 1,
            R - lam, R - lam - 1, R - lam + 1, half - (half % lam), half - (half % lam) + (lam >> 1),
            half - (half % lam) + (lam >> 1) + 1, half - (half % lam) - 1]
    vals += [(j * lam + d) % R for j in (2, 3, lam >> 1, (lam >> 1) - 1, lam - 1) for d in (-1, 0, 1, lam >> 1, (lam >> 1) + 1)]
    vals += [1 << b for b in (31, 32, 63, 64, 126, 127, 128, 191, 192, 253, 254)]
    return [v % R for v in vals]


def special_values() -> list:
    return list(M.SPECIALS.values()) + glv_boundaries()


def glv_split(k):
    """tests/test_abi.py glv_split: k = s (k1 + k2 lambda), the two signed halves."""
    s = -1 if k > (R - 1) // 2 else 1
    kp = R - k if s < 0 else k
    k2 = (kp + (GLV_LAMBDA >> 1)) // GLV_LAMBDA
    return s * (kp - k2 * GLV_LAMBDA), s * k2


def window_widths(c) -> list:
    """msm_plan.hip window_widths over the 127 bits of a half: as even as possible, the wider windows lowest."""
    w_count = (127 + c - 1) // c
    base, extra = divmod(127, w_count)
    return [base + (1 if w < extra else 0) for w in range(w_count)]


def nonzero_digits(v, widths) -> int:
    """Bucket entries one scalar becomes (k_digits): the non-zero digits of its two halves; the windows below the top are
    signed (a raw digit above half the range becomes its negative complement and carries one), the top one is not."""
    total = 0
    for h in glv_split(v):
        h, carry = abs(h), 0
        for w, c in enumerate(widths):
            r = (h & ((1 << c) - 1)) + carry
            h >>= c
            carry = 0
            if w != len(widths) - 1 and r > 1 << (c - 1):
                r, carry = (1 << c) - r, 1
            total += r != 0
    return total


def model_entries(rows, loose, c) -> int:
    """Sorted entries of one member-form call whose plan has window width c: zero scalars contribute nothing."""
    widths = window_widths(c)
    count = Counter(v for row, lo in zip(rows, loose) for v in list(row) + list(lo) if v)
    return sum(n * nonzero_digits(v, widths) for v, n in count.items())


def _inst_range(own, n_inst, j):
    return (WHISK_RANGE * j, WHISK_RANGE) if own else (0, n_inst)


def _shift(checks, crs_by, inst_by):
    return [k._replace(segs=tuple(s._replace(first=s.first + (crs_by if s.set == M.SET_CRS else inst_by)) for s in k.segs))
            for k in checks]


def _mid_case(rng, name, n_crs, n_inst, n_extra, k, own, families, carriers=None, uniform_len=None):
    """One description.  Roles (claims): `empty` members have nothing; `cancelling` has two FOLD checks with weights w and
    -w on the same slots; every worker has one CONST check over the whole CRS with a constant of its own, and only
    that check (and the cancelling pair) names CRS slots [0, N_EQ).  workers[0] has, besides it, nothing but a CONST check
    with the SAME constant a (1 + lambda) over its instance range: its halves k1 = k2 = a, so one bucket per window holds
    two entries per slot it names (in the Whisk shape 2 x 760 at L = 87: 18 fragments, over max_small = 16 -- no other
    segment of that shape is long enough for the large-bucket queue).  From four workers on the roles fall on different
    members; with fewer they pile up on the same ones."""
    b = M._Builder(rng)
    cmem = []
    hole = empties(k) if carriers is None else tuple(j for j in range(k) if j not in carriers)
    live = [j for j in range(k) if j not in hole]
    cancelling = live[-1] if "cancelling" in families else None
    workers = [j for j in live if j != cancelling]
    role = lambda i: workers[i % len(workers)]                       # noqa: E731
    claims = dict(shape=(n_crs, n_inst, n_extra, k), families=tuple(families), empty=hole, cancelling=cancelling,
                  workers=tuple(workers), all_equal={}, inst_const=None, few_values=None, specials=None, inf_inst=(),
                  exact_roles=len(workers) >= 4)

    def add(j, n_before):
        cmem.extend([j] * (len(b.checks) - n_before))

    for i, j in enumerate(workers):
        lo, ln = _inst_range(own, n_inst, j)
        if "all-equal" in families:
            a = M._fr(rng) >> 130                                     # below 2^125 < lambda / 2
            const = a * (1 + GLV_LAMBDA) % R if i == 0 else M._fr(rng)
            n0 = len(b.checks)
            b.check(M.CONST, n_crs, weight=const, segs=[(M.SET_CRS, 0, n_crs, 0)])
            claims["all_equal"][j] = const
            if i == 0 and ln:
                b.check(M.CONST, ln, weight=const, segs=[(M.SET_INST, lo, ln, 0)])
                claims["inst_const"] = (j, lo, ln)
                claims["inf_inst"] = (lo + 1, lo + 2, lo + 3)          # three instance slots whose scalar is not zero
            add(j, n0)
        if "uniform" in families and (i or len(workers) < 4 or "all-equal" not in families):
            n0 = len(b.checks)
            crs_n = n_crs - N_EQ
            inst_n = 0 if claims["exact_roles"] and j == role(2) else ln   # the specials member keeps its instance slots
            M._mixed_checks(b, rng, crs_n, inst_n, 2, max_len=uniform_len or max(crs_n, inst_n))
            b.checks[n0:] = _shift(b.checks[n0:], N_EQ, lo)
            add(j, n0)
    if "few-values" in families:
        j = role(1)
        lo, ln = _inst_range(own, n_inst, j)
        n = n_crs - N_EQ + ln
        m = M._ceil_log2(n)
        n0 = len(b.checks)                                            # w q, -w q^2, w q^3, +-w q^4: five values
        b.check(M.FOLD_POW, n, gammas=[1] * (m - 1) + [R - 1], q_cap=3,
                segs=[(M.SET_CRS, N_EQ, n_crs - N_EQ, 0), (M.SET_INST, lo, ln, n_crs - N_EQ)])
        claims["few_values"] = (j, n, 3)
        add(j, n0)
    if "specials" in families:
        j = role(2)
        lo, ln = _inst_range(own, n_inst, j)
        vals = special_values()
        n0 = len(b.checks)
        seg = (M.SET_INST, lo, len(vals), 0) if ln >= len(vals) else (M.SET_CRS, N_EQ, len(vals), 0)
        b.check(M.EXPLICIT, tail=vals, alpha=1, segs=[seg])
        claims["specials"] = (j, seg[0], seg[1], len(vals))
        add(j, n0)
    if cancelling is not None:
        lo, ln = _inst_range(own, n_inst, cancelling)
        n = n_crs + ln
        gam, w = M._frs(rng, M._ceil_log2(n)), M._fr(rng) or 1
        n0 = len(b.checks)
        for weight in (w, R - w):
            b.check(M.FOLD, n, gammas=gam, weight=weight, segs=[(M.SET_CRS, 0, n_crs, 0), (M.SET_INST, lo, ln, n_crs)])
        add(cancelling, n0)
    half = (R - 1) // 2
    xs = [R - 1, M._fr(rng), half, 0, GLV_LAMBDA, half + 1, 1, GLV_LAMBDA >> 1][:n_extra] if "loose" in families else []
    xs += M._frs(rng, n_extra - len(xs))
    xmem = [workers[e % len(workers)] for e in range(n_extra)]
    case = b.case(n_crs, n_inst, n_extra, f"{k} members over ({n_crs}, {n_inst}) + {n_extra}: {', '.join(families)}",
                  f"mid/{name}", extra_scalars=xs, inf_extra=1 if n_extra > 1 else -1)
    return case, cmem, xmem, claims


FAMILY_NAMES = ("uniform", "all-equal", "few-values", "specials", "cancelling", "loose")


def mid_cases(seed=2024) -> dict:
    """{name: (case, check_member, extra_member, claims)} over MID_SHAPES, every family at once in every shape: the triple
    of group_case and the dict of the case's claims.  claims["plan"] is what the shape is there for, claims["large"] whether
    the large-bucket queue must run; the other claims name the members of every role (_mid_case)."""
    out = {}
    for i, (name, n_crs, n_inst, n_extra, k, own, plan) in enumerate(MID_SHAPES):
        rng = np.random.default_rng([seed, i, n_crs, n_inst, k])
        case, cmem, xmem, claims = _mid_case(rng, name, n_crs, n_inst, n_extra, k, own, FAMILY_NAMES)
        claims["plan"] = plan
        claims["large"] = n_crs + n_inst >= 1100          # the large-bucket queue must run (an all-equal run > max_small x L)
        out[name] = (case, cmem, xmem, claims)
    return out


def uniform_control(seed=2024):
    """The many-1100-168 shape from the uniform family alone, as the control of the large-bucket queue: no bucket may
    reach it.  Segments of at most 8 slots: the longest run of equal scalars is one CONST check's six segments, 48 slots
    or 96 entries if both halves fall into one bucket; at L = 10 that is at most 11 fragments, below max_small = 16 (random
    scalars add a handful per bucket: 2,552 terms over at least 128 buckets per window, most of them zero)."""
    name, n_crs, n_inst, n_extra, k, own, plan = MID_SHAPES[2]
    rng = np.random.default_rng([seed, 99])
    case, cmem, xmem, claims = _mid_case(rng, "uniform-control", n_crs, n_inst, n_extra, k, own, ("uniform",), uniform_len=8)
    claims["plan"], claims["large"] = plan, False
    return case, cmem, xmem, claims


def last_accepted_case(seed=2024):
    """64 members over the largest CRS one pass of bucket slots takes (LAST_ACCEPTED), no instance points: the second,
    two middle and the second to last member carry an all-equal CONST check over the whole CRS, the last three of them
    two uniform checks besides; the other 60 have nothing."""
    n_crs, k = LAST_ACCEPTED["n_crs"], LAST_ACCEPTED["n_members"]
    carriers = (1, k // 2 - 1, k // 2, k - 2)
    rng = np.random.default_rng([seed, 77])
    case, cmem, xmem, claims = _mid_case(rng, "last-accepted", n_crs, 0, 0, k, False, ("uniform", "all-equal"), carriers=carriers)
    claims["carriers"] = carriers
    return case, cmem, xmem, claims


def mid_points(case, claims, base_pts, oracle):
    """(crs, inst, loose) of a mid case: case_points' tiling, then one point P on 64 CRS slots inside the all-equal segment,
    -P (y -> p - y on the limbs) on 32 more, and (0, 0) on the claimed instance slots.  curdle_dacc_begin takes an instance
    point at infinity (tests/dacc_model.py), so infinity is not kept to the loose pair."""
    crs, inst, loose = M.case_points(case, base_pts)
    p = base_pts[5].copy()
    neg = p.copy()
    neg[6:12] = oracle._limbs((oracle.P - oracle._from_limbs(p[6:12])) % oracle.P, 6)
    crs[list(P_SLOTS)] = p
    crs[list(NEG_SLOTS)] = neg
    for s in claims["inf_inst"]:
        inst[s] = 0
    return crs, inst, loose
