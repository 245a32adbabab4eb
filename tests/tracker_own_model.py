"""Does key k own a Whisk tracker?  The tracker of (k, r) is compress(r G) | compress(k r G) (the reference's
whisk/whisk_test.go:98-104, computeTracker); k owns a tracker (rG, krG) iff k rG and krG are the same group element,
infinity a group element like any other.  Big-integer affine arithmetic from oracle/py (scalar_mul, compress) on the
decoded points; nothing of the library.

The Python oracle has compress but no inverse, so gnark's G1Affine.SetBytes (curve and subgroup, whisk/types.go:85-95)
is restated here as `decompress`, with big integers: it raises ValueError where SetBytes errors."""
import glv_chain_model as M
from test_tracker_prove_gpu import bad_records

NOT_OWNED, OWNED, BAD = 0, 1, 2
_points = {}     # record bytes -> point, or ValueError
_products = {}   # (k, point) -> k * point


def decompress(oracle, rec):
    """48 bytes -> affine point or None (infinity); ValueError for what SetBytes refuses."""
    rec = bytes(rec)
    if rec not in _points:
        try:
            _points[rec] = _decompress(oracle, rec)
        except ValueError as e:
            _points[rec] = e
    if isinstance(_points[rec], ValueError):
        raise _points[rec]
    return _points[rec]


def _decompress(o, rec):
    if len(rec) != 48:
        raise ValueError("a compressed G1 point is 48 bytes")
    flags = rec[0] >> 5
    if not flags & 4:
        raise ValueError("uncompressed form")
    x = int.from_bytes(rec, "big") & ((1 << 381) - 1)
    if flags & 2:                                   # infinity: nothing else may be set
        if flags & 1 or x:
            raise ValueError("infinity with stray bits")
        return None
    if x >= o.P:
        raise ValueError("x >= p")
    rhs = (x * x * x + o.B_COEFF) % o.P
    y = pow(rhs, (o.P + 1) // 4, o.P)
    if y * y % o.P != rhs:
        raise ValueError("not on the curve")
    if (y > (o.P - 1) // 2) != bool(flags & 1):     # the flag names the lexicographically larger root
        y = o.P - y
    if o.scalar_mul(o.R, (x, y)) is not None:
        raise ValueError("not in the subgroup")
    return (x, y)


def product(oracle, k, pt):
    key = (k % oracle.R, pt)
    if key not in _products:
        _products[key] = oracle.scalar_mul(k % oracle.R, pt)
    return _products[key]


def owned(oracle, tracker_bytes, k):
    """True / False; ValueError if rG or krG does not decode."""
    assert len(tracker_bytes) == 96
    rG = decompress(oracle, tracker_bytes[:48])
    krG = decompress(oracle, tracker_bytes[48:])
    return product(oracle, k, rG) == krG


def verdict(oracle, tracker_bytes, k):
    """The batch's byte."""
    try:
        return OWNED if owned(oracle, tracker_bytes, k) else NOT_OWNED
    except ValueError:
        return BAD


def matrix(oracle, trackers, keys):
    """[len(keys)][len(trackers)] verdict bytes."""
    return [[verdict(oracle, t, k) for t in trackers] for k in keys]


def split_of(k, lam=M.LAMBDA, r=M.R):
    """(k1, k2) of the library's GLV split (csrc/bls12_381.h glv_split): k' = min(k, r - k), k2 = round(k' / lambda)."""
    kp = min(k % r, r - k % r)
    k2 = (kp + (lam >> 1)) // lam
    return kp - k2 * lam, k2


def case_families(oracle):
    """(keys, trackers): lists of (name, k) and (name, 96 bytes).  Three finite rG and infinity; about two dozen
    distinct trackers, ten more with a record that does not decode."""
    o, R, lam = oracle, oracle.R, M.LAMBDA
    rand = o.Rand(1616)
    half_only, lam_only = (lam >> 1) - 3, 5 * lam
    assert split_of(half_only)[1] == 0 and split_of(half_only)[0] != 0
    assert split_of(lam_only) == (0, 5)
    named = [("0", 0), ("1", 1), ("2", 2), ("r-1", R - 1), ("lambda", lam), ("lambda+1", lam + 1), ("r-lambda", R - lam),
             ("k2=0", half_only), ("k1=0", lam_only)]
    randoms = [("random %d" % j, rand.get_fr()) for j in range(4)]
    named_values = {k for _, k in named}
    keys = named + [("special %#x" % s, s) for s in M.special_scalars() if s not in named_values] + randoms

    bases = [o.scalar_mul(rand.get_fr(), o.G1) for _ in range(3)]
    inf = o.compress(None)

    def tracker(k, a):
        return o.compress(bases[a]) + o.compress(product(o, k, bases[a]))

    trackers = [("honest %s" % name, tracker(k, j % 3)) for j, (name, k) in enumerate(named + randoms[:2])]
    # "honest 0" is krG = infinity (owned by k = 0 alone); "honest 1" is rG = krG
    stranger = rand.get_fr()
    trackers += [("another key %d" % a, tracker(stranger + a, a)) for a in range(2)]
    for name, k, a in (("random 0", randoms[0][1], 1), ("lambda", lam, 2)):   # -(lambda rG) is (r - lambda) rG
        t = tracker(k, a)
        trackers.append(("krG negated, %s" % name, t[:48] + o.compress(o.neg(decompress(o, t[48:])))))
    trackers += [("rG = krG = infinity", inf + inf), ("rG = infinity, krG finite", inf + o.compress(bases[0])),
                 ("krG = infinity", o.compress(bases[1]) + inf)]
    good = tracker(randoms[2][1], 0)
    for name, rec in bad_records(o).items():
        trackers += [("bad rG: " + name, rec + good[48:]), ("bad krG: " + name, good[:48] + rec)]
    return keys, trackers
