"""A plain model of the device accumulator's slot scalars (include/curdle_msm.h, "Accumulator on the
device"): Python integers mod r, written from the header's definitions and the reference's
formulas -- innerproductargument.go:223-234 and samemultiscalarargument.go:267-277 (the folded
vectors), grandproductargument.go:234-242 (the capped powers of q), msmaccumulator.go:38-43 (slot +=
alpha * x_i) -- and NOT from csrc/dacc_eval.h: it builds whole vectors and adds them into the slots
check by check, where the kernel searches the checks per slot.  No GPU, no library.

Also here: the acceptance rules (validate), the routing between the four kernel builds (path), the
packing into the C ABI's arrays, and a deterministic generator of named case families, used by
tests/test_dacc_model.py (model against identities and against the host stand-in) and
tests/test_dacc_direct_gpu.py (kernels against the model).

Points at infinity: (0, 0) is accepted among the instance points and the loose points (the MSM's
conversion takes it as infinity); the generator puts one in each in the `totals` and `overlap`
families.  The resident CRS set is given finite points only.
"""
from typing import NamedTuple

import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

EXPLICIT, CONST, FOLD, FOLD_POW = 0, 1, 2, 3         # CURDLE_VEC_*
SET_CRS, SET_INST = 0, 1                             # CURDLE_SET_*
MAX_SEGS = 6                                         # CURDLE_DACC_MAX_SEGS
MAX_EXTRA = 16384                                    # CURDLE_DACC_MAX_EXTRA
CHECK_WORDS = 35                                     # sizeof(curdle_dacc_check) / 4: 11 fields + 6 segments of 4
KIND_NAMES = {EXPLICIT: "explicit", CONST: "const", FOLD: "fold", FOLD_POW: "fold_pow"}


class Seg(NamedTuple):
    set: int
    first: int
    len: int
    vec_first: int


class Check(NamedTuple):
    kind: int
    n_struct: int
    m: int
    q_cap: int
    weight_off: int
    alpha_off: int
    gammas_off: int
    q_off: int
    tail_off: int
    n_tail: int
    segs: tuple


class Case(NamedTuple):
    n_crs: int
    n_inst: int
    checks: list
    pool: list            # canonical integers < r
    n_extra: int
    what: str
    name: str = ""
    extra_scalars: tuple = ()
    inf_inst: int = -1    # index of an instance point replaced by (0, 0), or -1
    inf_extra: int = -1   # ... of a loose point
    tags: frozenset = frozenset()

    @property
    def n_res(self):
        return self.n_crs + self.n_inst

    @property
    def n_total(self):
        return self.n_res + self.n_extra


# ------------------------------------------------------------------------------- the vectors ---
def element(ck: Check, pool, i: int) -> int:
    """x[i] of a check without building the vector (indices up to 2^31 + n_tail)."""
    if i >= ck.n_struct:                              # explicit, multiplied by alpha (header: "on the device")
        return pool[ck.alpha_off] * pool[ck.tail_off + (i - ck.n_struct)] % R
    x = pool[ck.weight_off]                           # alpha * scale, folded in by the caller
    if ck.kind in (FOLD, FOLD_POW):
        j = 0
        while i >> j:                                 # prod over the set bits j of i of gammas[m-1-j]
            if (i >> j) & 1:
                x = x * pool[ck.gammas_off + ck.m - 1 - j] % R
            j += 1
    if ck.kind == FOLD_POW:
        x = x * pow(pool[ck.q_off], min(i, ck.q_cap) + 1, R) % R
    return x


def vector(ck: Check, pool) -> list:
    """The whole x vector of a check, the obvious way: the folded part as the iterated tensor
    product of (1, gamma) pairs cut to n_struct, powers of q by pow(), the tail times alpha."""
    w = pool[ck.weight_off]
    if ck.kind in (FOLD, FOLD_POW):
        v = _tensor(pool[ck.gammas_off:ck.gammas_off + ck.m], ck.n_struct)
        v = [w * a % R for a in v]
    elif ck.kind == CONST:
        v = [w] * ck.n_struct
    else:
        v = []
    if ck.kind == FOLD_POW:
        q = pool[ck.q_off]
        v = [a * pow(q, min(i, ck.q_cap) + 1, R) % R for i, a in enumerate(v)]
    a = pool[ck.alpha_off]
    return v + [a * t % R for t in pool[ck.tail_off:ck.tail_off + ck.n_tail]]


def _tensor(gammas, n):
    """(1, g_0) x (1, g_1) x ... x (1, g_{m-1}) cut to its first n elements.  The first factor varies
    slowest, so the first n <= 2^k elements are the product of the LAST k factors alone (the others
    contribute their 1): a vector of 1000 elements with m = 31 needs ten doublings, not 31."""
    k = _ceil_log2(n) if n else 0
    v = [1]
    for g in gammas[len(gammas) - k:] if k else []:
        v = [a * b % R for a in v for b in (1, g)]
    return v[:n]


def slots(checks, pool, n_crs, n_inst) -> list:
    """For each check, for each segment: slot[first + j] += x[vec_first + j]."""
    out = [0] * (n_crs + n_inst)
    for ck in checks:
        whole = vector(ck, pool) if ck.n_struct + ck.n_tail <= 4096 else None
        for sg in ck.segs:
            base = sg.first if sg.set == SET_CRS else n_crs + sg.first
            for j in range(sg.len):
                x = whole[sg.vec_first + j] if whole is not None else element(ck, pool, sg.vec_first + j)
                out[base + j] = (out[base + j] + x) % R
    return out


def exponents(checks) -> set:
    """Every exponent e = min(i, q_cap) + 1 that some slot of a FOLD_POW check raises q to."""
    out = set()
    for ck in checks:
        if ck.kind != FOLD_POW:
            continue
        for sg in ck.segs:
            for j in range(sg.len):
                i = sg.vec_first + j
                if i < ck.n_struct:
                    out.add(min(i, ck.q_cap) + 1)
    return out


# ------------------------------------------------------------------------------ the contract ---
def validate(checks, pool_len, n_crs, n_inst, n_extra) -> bool:
    """The acceptance rules of the header (the list under curdle_dacc_check) = dacc_submit_impl's."""
    if n_extra > MAX_EXTRA:
        return False
    for k in checks:
        if k.kind > FOLD_POW or len(k.segs) > MAX_SEGS or k.m > 31:
            return False
        if k.kind == EXPLICIT and k.n_struct:
            return False
        if k.n_struct > 1 << 31 or k.n_struct + k.n_tail >= 1 << 32:
            return False
        if k.weight_off >= pool_len or k.alpha_off >= pool_len or k.tail_off + k.n_tail > pool_len:
            return False
        if k.kind >= FOLD and k.gammas_off + k.m > pool_len:
            return False
        if k.kind == FOLD_POW and k.q_off >= pool_len:
            return False
        if k.kind >= FOLD and k.n_struct > 1 << k.m:
            return False
        for s in k.segs:
            if s.set not in (SET_CRS, SET_INST):
                return False
            if s.first + s.len > (n_crs if s.set == SET_CRS else n_inst):
                return False
            if s.vec_first + s.len > k.n_struct + k.n_tail:
                return False
        if any(not 0 <= v < 1 << 32 for v in k[:10]) or any(not 0 <= v < 1 << 32 for s in k.segs for v in s):
            return False
    return True


FUSED_MAX = 16384                  # dbases_api.hip, dacc_submit_impl: `const bool fused = n <= 16384;`
FRONT_BUDGET = (120 - 36) * 1024   # msm_sort_kernels.hip, launch_dacc_front: lds_bytes(.., kDaccFrontLds - 36 * 1024)
SPLIT_BUDGET = 120 * 1024          # dacc_kernels.hip: kDaccLdsBudget = 120 * 1024
CHECK_BYTES = 4 * CHECK_WORDS      # sizeof(curdle_dacc_check) in dacc_eval.h, lds_bytes


def lds_bytes(pool_len, n_checks, budget) -> int:
    """dacc_eval.h, lds_bytes: the pool, the checks rounded up to 16 bytes, 16 more; 0 = does not fit."""
    need = pool_len * 32 + (n_checks * CHECK_BYTES + 15) // 16 * 16 + 16
    return need if need <= budget else 0


def path(n_total, pool_len, n_checks) -> str:
    """Which of the four builds evaluates a call ("none": n = 0, infinity without a launch)."""
    if n_total == 0:
        return "none"
    if n_total <= FUSED_MAX:
        return "front_lds" if lds_bytes(pool_len, n_checks, FRONT_BUDGET) else "front_global"
    return "split_lds" if lds_bytes(pool_len, n_checks, SPLIT_BUDGET) else "split_global"


def largest_staged_pool(n_total, n_checks) -> int:
    """The largest pool_len that path() still stages at this size (the next one does not)."""
    staged = path(n_total, 0, n_checks)
    lo, hi = 0, 1 << 20
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if path(n_total, mid, n_checks) == staged else (lo, mid)
    return lo


# ---------------------------------------------------------------------------------- packing ---
def pack_checks(checks) -> np.ndarray:
    out = np.zeros((max(len(checks), 1), CHECK_WORDS), dtype=np.uint32)
    for c, k in enumerate(checks):
        out[c, :10] = k[:10]
        out[c, 10] = len(k.segs)
        for s, sg in enumerate(k.segs):
            out[c, 11 + 4 * s:15 + 4 * s] = sg
    return out[:len(checks)] if checks else out[:0]


def pack_fr(values, oracle) -> np.ndarray:
    """ints -> Montgomery fr.Element limbs, (n, 4) uint64."""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        out[i] = oracle.fr_to_mont_limbs(v)
    return out


def unpack_fr(limbs, oracle) -> list:
    return [oracle.fr_from_mont_limbs([int(x) for x in row]) for row in limbs]


def raw_ints(limbs) -> list:
    """The limbs as integers, unconverted (to check canonical form: each must be < r)."""
    return [sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in limbs]


def case_points(case: Case, base_pts: np.ndarray):
    """(crs, inst, loose) points of a case: a few hundred distinct points tiled to the sizes, the three
    sets starting at different places of the tile; the flagged ones replaced by (0, 0) = infinity."""
    def tile(n, start):
        return base_pts[(np.arange(n) + start) % len(base_pts)].copy() if n else np.zeros((0, 12), dtype=np.uint64)
    crs, inst, loose = tile(case.n_crs, 0), tile(case.n_inst, 101), tile(case.n_extra, 37)
    if case.inf_inst >= 0:
        inst[case.inf_inst] = 0
    if case.inf_extra >= 0:
        loose[case.inf_extra] = 0
    return crs, inst, loose


def as_map(oracle, pts, sc):
    """{base bytes: canonical scalar} with repeated bases merged; zero scalars and the point at
    infinity dropped (the reference's map keeps (0,0) as a key, the device never stores it)."""
    out = {}
    for p, s in zip(pts, sc):
        if not p.any():
            continue
        k = p.tobytes()
        out[k] = (out.get(k, 0) + oracle.fr_from_mont_limbs([int(v) for v in s])) % oracle.R
    return {k: v for k, v in out.items() if v}


# -------------------------------------------------------------------------------- generator ---
SPECIALS = {"0": 0, "1": 1, "2": 2, "r-1": R - 1, "r-2": R - 2, "(r-1)/2": (R - 1) // 2}
FAMILIES = ("kinds", "qpow", "tails", "overlap", "special", "totals", "routes", "random", "random_wide")


def _fr(rng) -> int:
    return int.from_bytes(rng.bytes(40), "big") % R


def _ceil_log2(n) -> int:
    k = 0
    while (1 << k) < n:
        k += 1
    return k


class _Builder:
    """Collects one case: a pool and checks that index it."""

    def __init__(self, rng):
        self.rng, self.pool, self.checks = rng, [], []

    def put(self, v) -> int:
        self.pool.append(v % R)
        return len(self.pool) - 1

    def check(self, kind, n_struct=0, gammas=(), tail=(), segs=(), q_cap=0, scale=None, alpha=None, q=None, m=None,
              weight=None):
        rng = self.rng
        alpha = _fr(rng) if alpha is None else alpha
        scale = _fr(rng) if scale is None else scale
        q = _fr(rng) if q is None else q
        self.put(_fr(rng))                                        # padding: offsets differ from one check to the next
        q_off = self.put(q)
        tail_off = len(self.pool)
        for t in tail:
            self.put(t)
        alpha_off = self.put(alpha)
        gammas_off = len(self.pool)
        for g in gammas:
            self.put(g)
        weight_off = self.put(alpha * scale if weight is None else weight)
        self.checks.append(Check(kind, n_struct, len(gammas) if m is None else m, q_cap, weight_off, alpha_off, gammas_off,
                                 q_off, tail_off, len(tail), tuple(Seg(*s) for s in segs)))

    def case(self, n_crs, n_inst, n_extra, what, name, extra_scalars=None, **kw) -> Case:
        if extra_scalars is None:
            extra_scalars = [_fr(self.rng) for _ in range(n_extra)]
        return Case(n_crs, n_inst, list(self.checks), list(self.pool), n_extra, what, name, tuple(extra_scalars), **kw)


def _frs(rng, n):
    return [_fr(rng) for _ in range(n)]


def _kinds(rng):
    for n in (1, 2, 3, 8, 13, 256, 1000):
        lg = _ceil_log2(n)
        shapes = [(EXPLICIT, 0), (CONST, 0), (CONST, 31)]
        for kind in (FOLD, FOLD_POW):
            shapes += [(kind, m) for m in sorted({0, lg, lg + 3, 31}) if n <= 1 << m]
        for idx, (kind, m) in enumerate(shapes):
            b = _Builder(rng)
            on_crs = (idx + n) % 2 == 0
            n_crs, n_inst = (n + 3, 5) if on_crs else (5, n + 3)
            seg = (SET_CRS if on_crs else SET_INST, 2, n, 0)
            if kind == EXPLICIT:
                b.check(EXPLICIT, tail=_frs(rng, n), segs=[seg])
            elif kind == CONST:
                b.check(CONST, n, gammas=_frs(rng, 2), m=m, segs=[seg])     # m is ignored for CONST
            else:
                b.check(kind, n, gammas=_frs(rng, m), segs=[seg], q_cap=int(rng.integers(0, n + 2)))
            yield b.case(n_crs, n_inst, 2, f"one {KIND_NAMES[kind]} check, one segment, n_struct={n}, m={m}",
                         f"{KIND_NAMES[kind]}-n{n}-m{m}")
    for kind in (FOLD, FOLD_POW):         # the last eight of 2^31 elements: products of up to 31 gammas
        b = _Builder(rng)
        b.check(kind, 1 << 31, gammas=_frs(rng, 31), segs=[(SET_INST, 1, 8, (1 << 31) - 8)], q_cap=0xFFFFFFFF)
        yield b.case(3, 9, 1, f"{KIND_NAMES[kind]}: indices 2^31-8 .. 2^31-1 of a vector of 2^31", f"{KIND_NAMES[kind]}-top-of-2p31")


QCAPS = (0, 1, 2, 3, 4, 7, 8, "n-1", "n", (1 << 31) - 1, (1 << 32) - 1)


def _qpow(rng):
    n = 20
    for cap in QCAPS:
        q_cap = {"n-1": n - 1, "n": n}.get(cap, cap)
        b = _Builder(rng)
        b.check(FOLD_POW, n, gammas=_frs(rng, 5), segs=[(SET_CRS, 0, n, 0)], q_cap=q_cap)
        yield b.case(n, 0, 1, f"q_cap={cap} over {n} elements", f"cap-{cap}")
    # windows round every power of two of a vector of 2^31 elements: e = 2^k - 2 .. 2^k + 1
    wins = [((1 << k) - 3, 4) for k in range(5, 31)] + [((1 << 31) - 4, 4)]
    for cap in ((1 << 32) - 1, (1 << 31) - 1, (1 << 20) + 5):
        b = _Builder(rng)
        gam, q = _frs(rng, 31), _fr(rng)
        for c in range(0, len(wins), MAX_SEGS):
            segs = [(SET_INST, 4 * (c + s), ln, vf) for s, (vf, ln) in enumerate(wins[c:c + MAX_SEGS])]
            b.check(FOLD_POW, 1 << 31, gammas=gam, segs=segs, q_cap=cap, q=q)
        yield b.case(2, 4 * len(wins), 0, f"exponents round 2^5 .. 2^31 with q_cap={cap}", f"windows-cap-{cap}")


def _tails(rng):
    spans = {"structured": (0, 6), "tail": (9, 7), "straddling": (5, 8), "all": (0, 16)}
    for kind in (CONST, FOLD, FOLD_POW):
        for where, (vf, ln) in spans.items():
            b = _Builder(rng)
            b.check(kind, 8, gammas=_frs(rng, 3), tail=_frs(rng, 8), segs=[(SET_CRS, 1, ln, vf)], q_cap=5)
            yield b.case(20, 3, 1, f"{KIND_NAMES[kind]}: a segment over the {where} part of 8 + 8", f"{KIND_NAMES[kind]}-{where}")
        b = _Builder(rng)
        b.check(kind, 8, gammas=_frs(rng, 3), segs=[(SET_INST, 0, 8, 0)], q_cap=9)
        yield b.case(2, 8, 0, f"{KIND_NAMES[kind]}: n_tail = 0", f"{KIND_NAMES[kind]}-no-tail")
        b = _Builder(rng)
        b.check(kind, 0, gammas=_frs(rng, 2), tail=_frs(rng, 5), segs=[(SET_INST, 1, 5, 0)])
        yield b.case(2, 8, 0, f"{KIND_NAMES[kind]}: n_struct = 0", f"{KIND_NAMES[kind]}-no-struct")
    b = _Builder(rng)
    b.check(EXPLICIT, tail=_frs(rng, 9), segs=[(SET_CRS, 0, 4, 5), (SET_INST, 0, 5, 0)])
    yield b.case(4, 5, 0, "explicit: two segments of one tail", "explicit-two-segments")
    b = _Builder(rng)
    b.check(FOLD_POW, 1 << 31, gammas=_frs(rng, 31), tail=_frs(rng, 8), segs=[(SET_CRS, 0, 8, (1 << 31) - 4)], q_cap=1 << 30)
    yield b.case(8, 0, 0, "a segment straddling the border at index 2^31", "straddling-2p31")


def _overlap(rng):
    b = _Builder(rng)
    b.check(FOLD_POW, 40, gammas=_frs(rng, 6), tail=_frs(rng, 8), q_cap=17,
            segs=[(SET_CRS, 10, 12, vf) for vf in (0, 1, 7, 28, 33, 36)])
    yield b.case(30, 2, 0, "six segments of one check on one slot range", "six-segments-one-range")
    b = _Builder(rng)
    for c in range(8):
        kind = (EXPLICIT, CONST, FOLD, FOLD_POW)[c % 4]
        b.check(kind, 0 if kind == EXPLICIT else 16, gammas=_frs(rng, 4), tail=_frs(rng, 24), segs=[(SET_INST, 3, 14, c)], q_cap=c)
    yield b.case(1, 20, 3, "eight checks on one slot range, an infinity among the instance and loose points",
                 "eight-checks-one-range", inf_inst=5, inf_extra=1)
    b = _Builder(rng)
    b.check(FOLD, 128, gammas=_frs(rng, 7), segs=[(SET_CRS, 250, 50, 3), (SET_INST, 0, 50, 53)])
    b.check(FOLD_POW, 100, gammas=_frs(rng, 7), tail=_frs(rng, 30), q_cap=70,
            segs=[(SET_INST, 20, 57, 60), (SET_CRS, 200, 100, 11), (SET_CRS, 299, 1, 0), (SET_INST, 0, 1, 129)])
    yield b.case(300, 77, 2, "one range of slots named through CRS and INST, n_crs = 300 not a multiple of the block",
                 "crs-inst-border")
    b = _Builder(rng)
    b.check(CONST, 4, segs=[(SET_CRS, 7, 4, 0)])
    b.check(EXPLICIT, tail=_frs(rng, 3), segs=[(SET_INST, 30, 3, 0)])
    b.check(FOLD, 4, gammas=_frs(rng, 2), segs=[])
    yield b.case(40, 40, 1, "most slots covered by no check (scalar 0), one check without segments", "uncovered-slots")
    b = _Builder(rng)
    b.check(CONST, 10, scale=1, alpha=5, segs=[(SET_CRS, 0, 10, 0)])
    b.check(CONST, 10, scale=1, alpha=R - 5, segs=[(SET_CRS, 0, 10, 0)])
    yield b.case(10, 0, 1, "two checks that cancel: every slot sums to 0 mod r", "cancelling-checks")


def _special(rng):
    roles = {EXPLICIT: ("alpha", "tail"), CONST: ("weight", "alpha", "tail"), FOLD: ("weight", "alpha", "tail", "gamma"),
             FOLD_POW: ("weight", "alpha", "tail", "gamma", "q")}
    for kind, rs in roles.items():
        for role in rs:
            for vname, v in SPECIALS.items():
                b = _Builder(rng)
                gam, tail = _frs(rng, 4), _frs(rng, 3)
                kw = {}
                if role == "alpha":
                    kw["alpha"] = v
                elif role == "weight":
                    kw["weight"] = v
                elif role == "q":
                    kw["q"] = v
                elif role == "gamma":
                    gam[int(rng.integers(4))] = v
                    gam[int(rng.integers(4))] = v
                else:
                    tail[int(rng.integers(3))] = v
                ns = 0 if kind == EXPLICIT else 13
                b.check(kind, ns, gammas=gam, tail=tail, segs=[(SET_CRS, 1, ns + 3, 0)], q_cap=int(rng.integers(0, 14)), **kw)
                xs = [v, _fr(rng)]
                yield b.case(ns + 5, 1, 2, f"{KIND_NAMES[kind]}: {role} = {vname}; a loose scalar = {vname}",
                             f"{KIND_NAMES[kind]}-{role}-{vname}", extra_scalars=xs,
                             tags=frozenset({(kind, role, vname)}))
    b = _Builder(rng)                                   # every constant special at once
    sp = list(SPECIALS.values())
    for c in range(6):
        b.check(FOLD_POW, 16, gammas=[sp[(c + j) % 6] for j in range(4)], tail=[sp[(c + j) % 6] for j in range(2)],
                alpha=sp[(c + 1) % 6] or 1, scale=sp[(c + 2) % 6], q=sp[(c + 3) % 6], q_cap=c, segs=[(SET_INST, 0, 18, 0)])
    yield b.case(0, 18, 6, "six checks whose every constant is special; special loose scalars", "all-special",
                 extra_scalars=sp)


def _mixed_checks(b, rng, n_crs, n_inst, n_checks, max_len=64):
    """n_checks random valid checks over the two sets."""
    for _ in range(n_checks):
        kind = int(rng.integers(4))
        m = int(rng.integers(0, 9))
        n_struct = 0 if kind == EXPLICIT else int(rng.integers(0, (1 << m) + 1)) if kind >= FOLD else int(rng.integers(0, 200))
        n_tail = int(rng.integers(0, 12))
        segs = []
        for _ in range(int(rng.integers(0, MAX_SEGS + 1))):
            st = int(rng.integers(2))
            set_n = n_crs if st == SET_CRS else n_inst
            ln = int(rng.integers(0, min(set_n, n_struct + n_tail, max_len) + 1))
            segs.append((st, int(rng.integers(0, set_n - ln + 1)), ln, int(rng.integers(0, n_struct + n_tail - ln + 1))))
        q_cap = int(rng.choice([0, 1, n_struct // 2, max(n_struct - 1, 0), n_struct, 0xFFFFFFFF, int(rng.integers(0, 300))]))
        b.check(kind, n_struct, gammas=_frs(rng, m), tail=_frs(rng, n_tail), segs=segs, q_cap=q_cap)


def _totals(rng):
    b = _Builder(rng)
    yield b.case(5, 4, 7, "no checks: loose pairs only over resident slots that all hold 0", "no-checks")
    b = _Builder(rng)
    _mixed_checks(b, rng, 9, 6, 3)
    yield b.case(9, 6, 0, "n_extra = 0", "no-loose-pairs")
    b = _Builder(rng)
    _mixed_checks(b, rng, 0, 12, 3)
    yield b.case(0, 12, 2, "n_crs = 0", "no-crs", inf_inst=11)
    b = _Builder(rng)
    _mixed_checks(b, rng, 12, 0, 3)
    yield b.case(12, 0, 2, "n_inst = 0", "no-inst", inf_extra=0)
    yield _Builder(rng).case(0, 0, 0, "n = 0: infinity without a launch", "nothing")
    yield _Builder(rng).case(0, 0, 3, "no resident slot at all: three loose pairs", "loose-only")
    b = _Builder(rng)
    b.check(CONST, 1, segs=[(SET_CRS, 0, 1, 0)])
    yield b.case(1, 0, 0, "one pair in all", "one-pair")
    for n_res, n_extra in ((1, 2), (255, 0), (256, 0), (257, 0), (511, 0), (513, 0), (255, 1), (255, 2), (256, 3)):
        b = _Builder(rng)
        n_crs = n_res * 2 // 3
        _mixed_checks(b, rng, n_crs, n_res - n_crs, 4, max_len=100)
        # ... and the last slots for sure: the lanes at the tail of the last block
        b.check(FOLD_POW, 8, gammas=_frs(rng, 3), segs=[(SET_INST, n_res - n_crs - 1, 1, 7)], q_cap=3)
        yield b.case(n_crs, n_res - n_crs, n_extra, f"n_res = {n_res}, n_extra = {n_extra}: the tail of a block", f"res{n_res}-extra{n_extra}")
    b = _Builder(rng)
    _mixed_checks(b, rng, 0, 0, 2)
    yield b.case(0, 0, MAX_EXTRA, "n_extra = CURDLE_DACC_MAX_EXTRA with no resident slot (n = 16384: fused)", "max-extra-alone")
    b = _Builder(rng)
    _mixed_checks(b, rng, 40, 30, 5)
    yield b.case(40, 30, MAX_EXTRA, "n_extra = CURDLE_DACC_MAX_EXTRA behind 70 resident slots (separate kernels)", "max-extra-behind-70")
    for n in (FUSED_MAX, FUSED_MAX + 1):
        b = _Builder(rng)
        _mixed_checks(b, rng, n - 300, 290, 6, max_len=100)
        b.check(FOLD, 16, gammas=_frs(rng, 4), segs=[(SET_CRS, n - 300 - 16, 16, 0), (SET_INST, 290 - 16, 16, 0)])
        yield b.case(n - 300, 290, 10, f"n = {n}: the fused / separate border", f"n{n}")


def _routes(rng):
    n_checks = 4
    for n in (FUSED_MAX, FUSED_MAX + 1):
        fit = largest_staged_pool(n, n_checks)
        for pool_len in (fit, fit + 1):
            n_extra = 33
            n_crs = n - n_extra - 700
            n_inst = 700
            b = _Builder(rng)
            b.check(FOLD_POW, 300, gammas=_frs(rng, 9), tail=_frs(rng, 20), q_cap=255,
                    segs=[(SET_CRS, 0, 200, 120), (SET_CRS, n_crs - 60, 60, 150), (SET_INST, 0, 40, 280)])
            b.check(FOLD, 512, gammas=_frs(rng, 11), segs=[(SET_CRS, n_crs // 2 - 3, 130, 380), (SET_INST, n_inst - 100, 100, 412)])
            b.check(CONST, 64, segs=[(SET_CRS, n_crs - 64, 64, 0), (SET_INST, n_inst - 64, 64, 0)])
            # a long tail brings the pool to its size; its LAST elements are the pool's last and are mapped to slots
            pad = pool_len - len(b.pool) - 4
            b.check(EXPLICIT, tail=_frs(rng, pad), segs=[(SET_INST, n_inst - 40, 40, pad - 40), (SET_CRS, 5, 40, 0)])
            # (_Builder.check puts alpha and the weight behind the tail: move the tail to the pool's end instead)
            ck = b.checks[-1]
            tail = b.pool[ck.tail_off:ck.tail_off + pad]
            rest = b.pool[ck.tail_off + pad:]
            b.pool[ck.tail_off:] = rest + tail
            sh = len(rest)
            b.checks[-1] = ck._replace(tail_off=ck.tail_off + sh, alpha_off=ck.alpha_off - pad, weight_off=ck.weight_off - pad,
                                       gammas_off=ck.gammas_off - pad)
            assert len(b.pool) == pool_len and len(b.checks) == n_checks
            yield b.case(n_crs, n_inst, n_extra, f"n = {n}, pool of {pool_len} elements: {path(n, pool_len, n_checks)}",
                         f"n{n}-pool{pool_len}", inf_extra=7)


def _random(rng, count=240):
    for i in range(count):
        big = i % 12 == 0       # (sizes thinned for the sanitizer build's textbook MSM: ~4 ms per non-zero slot)
        n_crs = int(rng.integers(0, 100 if big else 13))
        n_inst = int(rng.integers(0, 100 if big else 13))
        b = _Builder(rng)
        _mixed_checks(b, rng, n_crs, n_inst, int(rng.integers(0, 13)), max_len=50 if big else 12)
        yield b.case(n_crs, n_inst, int(rng.integers(0, 5)), "a random valid description", f"seed-case-{i}")


def _random_wide(rng, count=48):
    """Random descriptions at the sizes the small ones leave out: up to 600 resident slots (several 256-lane blocks
    of the fused front), long segments, up to 40 loose pairs.  Milliseconds for the C oracle; the sanitizer build's
    stand-in is given a handful of them only (tests/test_dacc_model.py)."""
    for i in range(count):
        n_crs, n_inst = int(rng.integers(60, 301)), int(rng.integers(60, 301))
        b = _Builder(rng)
        _mixed_checks(b, rng, n_crs, n_inst, int(rng.integers(1, 13)), max_len=300)
        yield b.case(n_crs, n_inst, int(rng.integers(0, 41)), "a random valid description over several blocks", f"seed-case-{i}")


_GEN = {"kinds": _kinds, "qpow": _qpow, "tails": _tails, "overlap": _overlap, "special": _special, "totals": _totals,
        "routes": _routes, "random": _random, "random_wide": _random_wide}


def family(name: str, seed: int = 2024) -> list:
    """The cases of one family, the same on every call: (n_crs, n_inst, checks, pool, n_extra, what, ...)."""
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    return [c._replace(name=f"{name}/{c.name}") for c in _GEN[name](rng)]


def all_cases(seed: int = 2024) -> list:
    return [c for f in FAMILIES for c in family(f, seed)]


def stand_in_cost(case: Case) -> int:
    """Scalar multiplications the naive host stand-in spends on a case (non-zero slots + loose pairs)."""
    covered = set()
    for ck in case.checks:
        for sg in ck.segs:
            base = sg.first if sg.set == SET_CRS else case.n_crs + sg.first
            covered.update(range(base, base + sg.len))
    return len(covered) + case.n_extra


def pack_case_file(cases, base_pts, oracle, two_step=False) -> bytes:
    """The flat binary that `host_flow dacc <file>` reads (tests/hostbuild/host_flow.cpp, Dacc)."""
    out = [np.array([len(cases)], dtype=np.uint64).tobytes()]
    for c in cases:
        crs, inst, loose = case_points(c, base_pts)
        out.append(np.array([c.n_crs, c.n_inst, len(c.checks), len(c.pool), c.n_extra, int(two_step)], dtype=np.uint64).tobytes())
        out += [pack_checks(c.checks).tobytes(), pack_fr(c.pool, oracle).tobytes(), crs.tobytes(), inst.tobytes(), loose.tobytes(),
                pack_fr(c.extra_scalars, oracle).tobytes()]
    return b"".join(out)


def parse_case_output(text: str):
    """[(rc, [exported Montgomery integers], [18 words of the sum] or None)] from `host_flow dacc`'s output."""
    res = []
    for line in text.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "case":
            res.append([int(w[3]), [], None])
        elif w[0] == "s":
            res[-1][1].append(int(w[1], 16))
        elif w[0] == "sum":
            res[-1][2] = [int(x, 16) for x in w[1:]]
    return res
