"""GenerateWhiskTrackerProof (the reference's whisk/whisk.go:149-175) for one member, with big integers:

    kG = k G,  A = b G,  B = b rG                                    (:156-159)
    c  = Transcript("whisk_opening_proof") . AppendPoints("tracker_opening_proof", kG g1Gen krG rG A B)
                                           . GetAndAppendChallenge("tracker_opening_proof_challenge")   (:161-169)
    s  = b - c k  in Fr                                              (:171-172)
    proof = compress(A) | compress(B) | s as 32 big-endian bytes     (types.go:119-128)

from oracle/py (scalar_mul, compress) and tests/merlin_model.py; nothing of the library.  The tracker of (k, r) is
compress(r G) | compress(k r G) (whisk_test.go:98-104)."""
import merlin_model as mm

LABEL = b"whisk_opening_proof"
PROGRAM = [(mm.TR_APPEND, b"tracker_opening_proof", 6, 48), (mm.TR_CHALLENGES, b"tracker_opening_proof_challenge", 1, 0)]


class Model:
    """Keeps the points of the (k, r) pairs it has seen: the GPU tests tile a small pool with fresh blinders."""

    def __init__(self, oracle):
        self.o = oracle
        self.gen = oracle.compress(oracle.G1)
        self._pairs = {}

    def pair(self, k, r):
        """(rG as a point, tracker bytes, compress(kG))"""
        key = (k, r)
        if key not in self._pairs:
            o = self.o
            rG = o.scalar_mul(r % o.R, o.G1)
            tracker = o.compress(rG) + o.compress(o.scalar_mul(k % o.R, rG))
            self._pairs[key] = (rG, tracker, o.compress(o.scalar_mul(k % o.R, o.G1)))
        return self._pairs[key]

    def tracker(self, k, r):
        return self.pair(k, r)[1]

    def k_commitment(self, k, r):
        return self.pair(k, r)[2]

    def proof(self, k, r, b):
        o = self.o
        rG, tracker, kG = self.pair(k, r)
        A = o.compress(o.scalar_mul(b % o.R, o.G1))
        B = o.compress(o.scalar_mul(b % o.R, rG))
        row = kG + self.gen + tracker[48:] + tracker[:48] + A + B
        challenges, _, _, status, _ = mm.run_program(PROGRAM, row, LABEL)
        assert status == 0 and len(challenges) == 1
        c = int.from_bytes(challenges[0], "big")
        s = (b - c * k) % o.R
        return A + B + s.to_bytes(32, "big")


# The case families of the single call and of the batch: (name, k, r); every one is an honest member.
def case_families(oracle):
    R = oracle.R
    rand = oracle.Rand(1414)
    cases = [("random %d" % j, rand.get_fr(), rand.get_fr()) for j in range(3)]
    cases += [("k=0", 0, rand.get_fr()), ("k=1", 1, rand.get_fr()), ("k=r-1", R - 1, rand.get_fr()),
              ("r=1", rand.get_fr(), 1), ("tracker=inf", rand.get_fr(), 0)]
    return cases
