"""A scalar-domain model of the GLV double-and-add chains on quads (go-curdleproofs_amd/csrc/glv_quad.h):
the single chain of k_scalar_mul_batch_quad (group_kernels.hip) and the joint chain of k_tracker_check
(tracker_kernels.hip).  Every point of a chain is a multiple of ONE point P, so the chain is replayed on
integers mod r, with no curve arithmetic: the state u stands for acc = u P.

Per bit 126..0 the state doubles, then every table of the chain (in the kernel's order) whose halves
have a bit set adds v = k_t (sa ba + sb bb lambda): the halves and their signs come from the split the
kernels run (curdle_selftest_op operation 11, splits() below), k_t is 1 for the table of P and k for
the table of Q = k P.  What q28::add (quad28.h) does with the operands is decided in its order:

    adds-infinity   the addend is infinity (k = 0, or P itself is infinity): add() returns at once
    into-infinity   u = 0: the sum is a copy of the addend
    equal           u = v: the doubling branch
    opposite        u = -v: the sum becomes infinity in the middle of the chain
    plain           anything else

The final addition of -T (the tracker check's comparison) is recorded the same way, at bit -1.

Why the single chain never meets `equal` or `opposite` (tests/test_glv_chain_model.py checks it, part b):
before the addition at bit j the state is u = X + Y lambda with X = 2 sa (a >> (j + 1)), Y = 2 sb (b >> (j + 1))
as plain integers, and the addend is v = x + y lambda with x, y in {0, +-1}.  u = +-v (mod r) makes
(X -+ x, Y -+ y) a vector of the lattice {(m, n): m + n lambda = 0 mod r}, whose nonzero vectors have a
coordinate of size lambda or more (it is spanned by (-lambda, 1) and (1, lambda + 1)), while the halves of
a reduced split stay below lambda / 2 + 1: the vector is zero, and X = +-x, Y = +-y with X, Y even and not
both zero is impossible.  The joint chain has no such protection: Q is a known multiple of P."""
import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF      # z^2 - 1: lambda^2 + lambda + 1 = r (tests/test_abi.py GLV_LAMBDA)
BITS = 127

PLAIN, EQUAL, OPPOSITE, INTO_INF, ADDS_INF = "plain", "equal", "opposite", "into-infinity", "adds-infinity"
SITE_S, SITE_C, SITE_T = "s", "c", "final"
FINAL_BIT = -1

# The scalar whose split has the largest half among the cases of tests/test_abi.py
# test_the_c_split_routine_against_big_integer_division (glv_split_cases(R, 300_000, 11));
# tests/test_glv_chain_model.py finds it again.
LARGEST_HALF_SCALAR = 0x39F6D3A994CEBEA4199CEC0404D0EC0253BC0000FFFE5BFE7FFFFFFF00000001   # a half of (lambda + 1) / 2


def splits(cm, scalars, on_device):
    """[(a, b, sign_a, sign_b)] of canonical scalars through operation 11: the split the kernels run, in
    its host build (on_device False) or its device build.  Signs are +1 / -1."""
    words = np.array([[(int(v) >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for v in scalars], dtype=np.uint32)
    words = words.reshape(len(scalars), 8)
    out = cm.selftest_op(11, words, on_device) if len(scalars) else np.zeros((0, 10), dtype=np.uint32)
    res = []
    for o in out:
        a = sum(int(o[j]) << (32 * j) for j in range(4))
        b = sum(int(o[4 + j]) << (32 * j) for j in range(4))
        assert int(o[8]) in (0, 0x80000000) and int(o[9]) in (0, 0x80000000)
        assert a < 1 << BITS and b < 1 << BITS
        res.append((a, b, -1 if int(o[8]) else 1, -1 if int(o[9]) else 1))
    return res


def classify(u, v, addend_is_infinity):
    """The branch q28::add takes for acc = u P and the addend v P, in add()'s own order."""
    if addend_is_infinity:
        return ADDS_INF
    if u == 0:
        return INTO_INF
    if u == v:
        return EQUAL
    if (u + v) % R == 0:
        return OPPOSITE
    return PLAIN


def addend(split, bit, k_t=1, lam=LAMBDA):
    """The scalar of the table entry the chain picks at `bit` (None: both bits clear, nothing is added)."""
    a, b, sa, sb = split
    ba, bb = (a >> bit) & 1, (b >> bit) & 1
    if not (ba or bb):
        return None
    return k_t * (sa * ba + sb * bb * lam) % R


def chain(tables, t=None, t_is_infinity=False, lam=LAMBDA):
    """tables: [(site, split, k_t, infinite)] in the kernel's order.  Returns ([(bit, site, class)], u) with
    u the state after bit 0, before the final addition of -t P (recorded at FINAL_BIT when t is given)."""
    events, u = [], 0
    for bit in range(BITS - 1, -1, -1):
        u = 2 * u % R
        for site, split, k_t, infinite in tables:
            v = addend(split, bit, k_t, lam)
            if v is None:
                continue
            events.append((bit, site, classify(u, v, infinite)))
            if not infinite:
                u = (u + v) % R
    if t is not None:
        events.append((FINAL_BIT, SITE_T, classify(u, -t % R, t_is_infinity)))
    return events, u


def single_chain(split, lam=LAMBDA):
    """k_scalar_mul_batch_quad on a finite point."""
    return chain([(SITE_S, split, 1, False)], lam=lam)


def joint_chain(s_split, c_split, k, t=None, p_is_infinity=False, lam=LAMBDA):
    """One chain of k_tracker_check: acc = s P + c Q with Q = k P, then acc - T with T = t P.  The units are
    multiples of P, so chain 0 (P = G, T = A) and chain 1 (P = rG, T = B) of an honest member share one trace
    unless rG is infinity (p_is_infinity: every table entry and T are infinity)."""
    k %= R
    tables = [(SITE_S, s_split, 1, p_is_infinity), (SITE_C, c_split, k, p_is_infinity or k == 0)]
    return chain(tables, t, p_is_infinity or (t is not None and t % R == 0), lam)


def exceptional(events):
    """The steps of a trace that take the equal or the opposite branch."""
    return [e for e in events if e[2] in (EQUAL, OPPOSITE)]


def single_chains_have_no_exceptional_step(split_list, scalars, lam=LAMBDA):
    """Part (b) for many scalars at once (numpy arrays of Python integers, one chain per element): returns the
    indices of the scalars whose single chain meets `equal` or `opposite` or does not end on the scalar.
    The same recurrence as chain(), which the caller runs on whatever this reports."""
    n = len(split_list)
    a = np.array([s[0] for s in split_list], dtype=object)
    b = np.array([s[1] for s in split_list], dtype=object)
    v1 = np.array([s[2] % R for s in split_list], dtype=object)
    v2 = np.array([s[3] * lam % R for s in split_list], dtype=object)
    v3 = (v1 + v2) % R
    zero = np.zeros(n, dtype=object)
    u = np.zeros(n, dtype=object)
    bad = np.zeros(n, dtype=bool)
    for bit in range(BITS - 1, -1, -1):
        u = (u + u) % R
        ba = ((a >> bit) & 1).astype(bool)
        bb = ((b >> bit) & 1).astype(bool)
        v = np.where(ba & bb, v3, np.where(ba, v1, np.where(bb, v2, zero)))
        any_bit = ba | bb
        nonzero = (u != 0).astype(bool)
        bad |= any_bit & nonzero & (u == v).astype(bool)              # equal
        u = (u + v) % R
        bad |= any_bit & nonzero & (u == 0).astype(bool)              # opposite: the sum is zero
    bad |= (u != np.array([int(s) % R for s in scalars], dtype=object)).astype(bool)
    return [int(i) for i in np.nonzero(bad)[0]]


def special_scalars(extra=()):
    """The list S of the single chain's tests: the boundaries of the split, with the scalars
    tests/test_msm_gpu.py test_scalars_at_the_boundaries_of_the_split uses and LARGEST_HALF_SCALAR."""
    lam, half = LAMBDA, (R - 1) // 2
    vals = [0, 1, 2, R - 1, R - 2,
            lam, lam + 1, lam - 1, R - lam, R - lam + 1, R - lam - 1, lam * lam % R,
            (R + 1) // 2, (R - 1) // 2,
            1 << 126, 1 << 127, (1 << 127) + 1, (1 << 127) - 1, (1 << 128) - 1, 1 << 254]
    vals += [a * (1 + lam) % R for a in (1, 2, 1 << 64)]               # equal halves
    # test_scalars_at_the_boundaries_of_the_split
    vals += [0, 1, 2, R - 1, R - 2, half, half + 1, half - 1, lam, lam - 1, lam + 1, lam >> 1, (lam >> 1) + 1, (lam >> 1) - 1,
             R - lam, R - lam - 1, R - lam + 1, half - (half % lam), half - (half % lam) + (lam >> 1),
             half - (half % lam) + (lam >> 1) + 1, half - (half % lam) - 1]
    vals += [(j * lam + d) % R for j in (2, 3, lam >> 1, (lam >> 1) - 1, lam - 1) for d in (-1, 0, 1, lam >> 1, (lam >> 1) + 1)]
    vals += [1 << e for e in (31, 32, 63, 64, 126, 127, 128, 191, 192, 253, 254)]
    vals.append(LARGEST_HALF_SCALAR)
    vals += list(extra)
    seen, out = set(), []
    for v in vals:
        v %= R
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


# The tracker check's k values (the multiples Q = k P a search runs over)
TRACKER_KS = [1, R - 1, 2, R - 2, (R + 1) // 2, (R - 1) // 2, LAMBDA, R - LAMBDA, LAMBDA + 1, LAMBDA * LAMBDA % R, 0]
