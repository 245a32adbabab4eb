"""Big-integer model of the combined tracker check (curdle_whisk_is_valid_tracker_proof_batch_combined): the
coefficients, the 5 k MSM scalars and the generator's scalar, the exclusion rule, and the weighted sum itself over the
oracle's points, with every challenge from the plain model of Merlin.  Not a test module.

    rho_i | sigma_i = SHAKE256("curdle/tracker-combine/v1" | seed | le64(i))[0:32], two little-endian 128-bit integers
    scalars of member i (rG, krG, kG, A, B):  sigma s, sigma c, rho c, -rho, -sigma   (mod r; all zero when excluded)
    g = sum rho_i s_i mod r over the members that are not excluded
    sum = g G + sum_i sum_j scalar_ij record_ij

It also makes members that are individually INVALID but whose errors cancel under equal coefficients, from known
discrete logs: a cancelling pair and a self-cancelling member."""
import hashlib
from collections import namedtuple

import merlin_model as mm

DOMAIN = b"curdle/tracker-combine/v1"
LABEL = b"whisk_opening_proof"
PROGRAM = [(mm.TR_APPEND, b"tracker_opening_proof", 6, 48), (mm.TR_CHALLENGES, b"tracker_opening_proof_challenge", 1, 0)]

# bytes: (tracker, k commitment, proof) as the C ABI takes them; points: (rG, krG, kG, A, B) as oracle points, or None
# where the member is only known by its bytes; s, c: response and challenge; excluded: the library answers CURDLE_EINVAL
Member = namedtuple("Member", "bytes points s c excluded")

_challenges = {}


def coefficients(seed: bytes, i: int):
    assert len(seed) == 32
    out = hashlib.shake_256(DOMAIN + seed + i.to_bytes(8, "little")).digest(32)
    return int.from_bytes(out[:16], "little"), int.from_bytes(out[16:], "little")


def equal_coefficients(seed: bytes, i: int):
    """What an attacker who could predict the coefficients would wish for."""
    return 1, 1


def challenge(oracle, tracker: bytes, kc: bytes, proof: bytes) -> int:
    """whisk.go:131-134 over the member's bytes: kG | g1Gen | krG | rG | A | B."""
    key = (tracker, kc, proof[:96])
    if key not in _challenges:
        row = kc + oracle.compress(oracle.G1) + tracker[48:] + tracker[:48] + proof[:96]
        ch, _, _, status, _ = mm.run_program(PROGRAM, row, LABEL)
        assert status == 0 and len(ch) == 1
        _challenges[key] = int.from_bytes(ch[0], "big")
    return _challenges[key]


def member_from_bytes(oracle, tracker: bytes, kc: bytes, proof: bytes, excluded: bool, points=None) -> Member:
    """A member known by its bytes: `excluded` is what the single call says (CURDLE_EINVAL), S >= r included."""
    s = int.from_bytes(proof[96:], "big")
    excluded = bool(excluded) or s >= oracle.R
    return Member((tracker, kc, proof), points, s, challenge(oracle, tracker, kc, proof), excluded)


def member_from_points(oracle, rG, krG, kG, A, B, s_of_c) -> Member:
    """A member from its five points; s_of_c(c) gives the response once the transcript has given the challenge."""
    tracker = oracle.compress(rG) + oracle.compress(krG)
    kc = oracle.compress(kG)
    ab = oracle.compress(A) + oracle.compress(B)
    c = challenge(oracle, tracker, kc, ab + bytes(32))
    s = s_of_c(c) % oracle.R
    return Member((tracker, kc, ab + s.to_bytes(32, "big")), (rG, krG, kG, A, B), s, c, False)


def honest_member(oracle, k: int, r: int, b: int) -> Member:
    """GenerateWhiskTrackerProof (whisk.go:149-175) with blinder b: A = b G, B = b rG, s = b - c k."""
    G = oracle.G1
    rG = oracle.scalar_mul(r % oracle.R, G)
    return member_from_points(oracle, rG, oracle.scalar_mul(k % oracle.R, rG), oracle.scalar_mul(k % oracle.R, G),
                              oracle.scalar_mul(b % oracle.R, G), oracle.scalar_mul(b % oracle.R, rG), lambda c: b - c * k)


def honest_points(oracle, k: int, r: int, b: int):
    """The five points of the honest member with these discrete logs (to pair with bytes the library produced)."""
    G = oracle.G1
    rG = oracle.scalar_mul(r % oracle.R, G)
    return (rG, oracle.scalar_mul(k % oracle.R, rG), oracle.scalar_mul(k % oracle.R, G),
            oracle.scalar_mul(b % oracle.R, G), oracle.scalar_mul(b % oracle.R, rG))


def off_by(oracle, k: int, r: int, a: int, b2: int) -> Member:
    """A = a G, B = b' rG, s = b' - c k: equation 2 holds, equation 1 is off by (b' - a) G."""
    G = oracle.G1
    rG = oracle.scalar_mul(r, G)
    return member_from_points(oracle, rG, oracle.scalar_mul(k, rG), oracle.scalar_mul(k, G), oracle.scalar_mul(a, G),
                              oracle.scalar_mul(b2, rG), lambda c: b2 - c * k)


def cancelling_pair(oracle, d: int = 0x1234567):
    """Two invalid members whose first equations are off by +d G and -d G."""
    return (off_by(oracle, k=0x51, r=0x77, a=1000, b2=1000 + d), off_by(oracle, k=0x93, r=0x35, a=5000 + d, b2=5000))


def self_cancelling(oracle, k: int = 0x29, a: int = 300, b2: int = 900) -> Member:
    """Over a tracker with rG = G: A = a G, B = b' G, s = (a + b')/2 - c k; the equations are off by +-(b' - a)/2 G."""
    G = oracle.G1
    kG = oracle.scalar_mul(k, G)
    half = pow(2, -1, oracle.R)
    return member_from_points(oracle, G, kG, kG, oracle.scalar_mul(a, G), oracle.scalar_mul(b2, G),
                              lambda c: (a + b2) * half - c * k)


def equation_errors(oracle, m: Member):
    """(s G + c kG - A, s rG + c krG - B): both infinity iff the single call accepts."""
    rG, krG, kG, A, B = m.points
    e1 = oracle.add(oracle.add(oracle.scalar_mul(m.s, oracle.G1), oracle.scalar_mul(m.c, kG)), oracle.neg(A))
    e2 = oracle.add(oracle.add(oracle.scalar_mul(m.s, rG), oracle.scalar_mul(m.c, krG)), oracle.neg(B))
    return e1, e2


def scalars_and_g(oracle, members, seed: bytes, first: int = 0, coeff=coefficients):
    """([5 canonical scalars per member], g); member j of the list is member first + j of the call."""
    R = oracle.R
    out, g = [], 0
    for j, m in enumerate(members):
        if m.excluded:
            out.append((0, 0, 0, 0, 0))
            continue
        rho, sigma = coeff(seed, first + j)
        out.append((sigma * m.s % R, sigma * m.c % R, rho * m.c % R, -rho % R, -sigma % R))
        g = (g + rho * m.s) % R
    return out, g


def mont_limbs(oracle, scalars):
    """The scalars as the kernel writes them: [k][5][4] Montgomery limbs."""
    return [[[int(v) for v in oracle.fr_to_mont_limbs(x)] for x in five] for five in scalars]


def weighted_sum(oracle, members, seed: bytes, first: int = 0, coeff=coefficients):
    """The MSM of the combined pass, over the oracle's points."""
    scalars, g = scalars_and_g(oracle, members, seed, first, coeff)
    acc = oracle.scalar_mul(g, oracle.G1)
    for m, five in zip(members, scalars):
        if m.excluded:  # zero scalars: its records, which may not be points at all, never enter
            assert five == (0, 0, 0, 0, 0)
            continue
        for pt, x in zip(m.points, five):
            acc = oracle.add(acc, oracle.scalar_mul(x, pt))
    return acc
