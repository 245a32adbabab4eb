"""A big-integer-style model of the batched Merlin transcripts (curdle_transcript_batch / _host): Keccak-f[1600],
the STROBE-128 subset Merlin uses (meta-AD, AD, PRF), Merlin's framing and the reference wrapper's
GetAndAppendChallenge with its retries (transcript.go:48-58), in plain Python over bytes and integers -- nothing
shared with host/transcript.cpp or the kernel.  Pure-Python Keccak costs a few tenths of a millisecond per
permutation: keep it to small shapes.

run_program() is the model of one member.  positions() replays a program's positions alone (they do not depend on
data), which is what the generator of the boundary programs searches with."""
import hashlib

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001      # the BLS12-381 scalar field
STATE_SIZE = 208
TR_APPEND, TR_CHALLENGES = 1, 2
MAX_TRIES = 256
RATE = 166
FLAG_I, FLAG_A, FLAG_C, FLAG_M, FLAG_K = 1, 2, 4, 16, 32

_RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808a, 0x8000000080008000, 0x000000000000808b,
       0x0000000080000001, 0x8000000080008081, 0x8000000000008009, 0x000000000000008a, 0x0000000000000088,
       0x0000000080008009, 0x000000008000000a, 0x000000008000808b, 0x800000000000008b, 0x8000000000008089,
       0x8000000000008003, 0x8000000000008002, 0x8000000000000080, 0x000000000000800a, 0x800000008000000a,
       0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
_M64 = (1 << 64) - 1


def _rho_offsets():
    """FIPS 202 section 3.2.2: the offsets of rho by walking (x, y) -> (y, 2x + 3y) from (1, 0)."""
    off = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        off[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return off


_RHO = _rho_offsets()


def keccak_f1600(lanes):
    """The permutation on 25 lanes, lane (x, y) at index x + 5 y (FIPS 202 section 3.2, written from the definition)."""
    a = list(lanes)
    for rc in _RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x - 1) % 5] ^ (((c[(x + 1) % 5] << 1) | (c[(x + 1) % 5] >> 63)) & _M64) for x in range(5)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                v = a[x + 5 * y] ^ d[x]
                r = _RHO[x][y]
                if r:
                    v = ((v << r) | (v >> (64 - r))) & _M64
                b[y + 5 * ((2 * x + 3 * y) % 5)] = v
        for y in range(0, 25, 5):
            for x in range(5):
                a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & _M64 & b[y + (x + 2) % 5])
        a[0] ^= rc
    return a


def permute_bytes(state: bytearray) -> None:
    lanes = [int.from_bytes(state[8 * i: 8 * i + 8], "little") for i in range(25)]
    state[:] = b"".join(v.to_bytes(8, "little") for v in keccak_f1600(lanes))


def sponge(msg: bytes, rate: int, suffix: int, out_len: int) -> bytes:
    """The FIPS 202 sponge over the model's permutation (SHA3-256: rate 136, suffix 0x06; SHAKE256: rate 136, 0x1f)."""
    st = bytearray(200)
    m = bytearray(msg) + bytes([suffix])
    m += bytes(-len(m) % rate)
    m[-1] ^= 0x80
    for at in range(0, len(m), rate):
        for i in range(rate):
            st[i] ^= m[at + i]
        permute_bytes(st)
    out = b""
    while len(out) < out_len:
        out += bytes(st[:rate])
        if len(out) < out_len:
            permute_bytes(st)
    return out[:out_len]


class Strobe:
    """STROBE-128/1600 as Merlin uses it.  hashing=False replays the positions alone.  `events` collects what the
    boundary tests ask about: (name, ...) tuples, see boundary_programs()."""

    def __init__(self, protocol: bytes = None, hashing=True, exported: bytes = None):
        self.hashing = hashing
        self.events = []
        self.permutations = 0
        if exported is not None:
            assert len(exported) == STATE_SIZE and exported[203:] == bytes(5)
            self.st = bytearray(exported[:200])
            self.pos, self.pos_begin, self.cur_flags = exported[200], exported[201], exported[202]
            return
        self.st = bytearray(200)
        self.st[0:6] = bytes([1, RATE + 2, 1, 0, 1, 96])
        self.st[6:18] = b"STROBEv1.0.2"
        self._permute()
        self.pos = self.pos_begin = self.cur_flags = 0
        self.meta_ad(protocol, False)

    def export(self) -> bytes:
        return bytes(self.st) + bytes([self.pos, self.pos_begin, self.cur_flags, 0, 0, 0, 0, 0])

    def _permute(self):
        self.permutations += 1
        if self.hashing:
            permute_bytes(self.st)

    def _run_f(self):
        self.st[self.pos] ^= self.pos_begin
        self.st[self.pos + 1] ^= 0x04
        self.st[RATE + 1] ^= 0x80
        self._permute()
        self.pos = self.pos_begin = 0

    def _absorb(self, data: bytes):
        for b in data:
            self.st[self.pos] ^= b
            self.pos += 1
            if self.pos == RATE:
                self._run_f()

    def _squeeze(self, n: int) -> bytes:
        out = bytearray()
        for _ in range(n):
            out.append(self.st[self.pos])
            self.st[self.pos] = 0
            self.pos += 1
            if self.pos == RATE:
                self._run_f()
        return bytes(out)

    def _begin_op(self, flags: int, more: bool):
        if more:
            assert flags == self.cur_flags
            return
        if self.pos == RATE - 1:
            self.events.append(("header_straddles", flags))
        old = self.pos_begin
        self.pos_begin = self.pos + 1
        self.cur_flags = flags
        self._absorb(bytes([old, flags]))
        if flags & (FLAG_C | FLAG_K):
            if self.pos != 0:
                self._run_f()
            else:
                self.events.append(("header_ends_at_166_no_forced_f", flags))

    def meta_ad(self, data: bytes, more: bool):
        self._begin_op(FLAG_M | FLAG_A, more)
        if more and len(data) == 4 and RATE - 4 < self.pos < RATE:
            self.events.append(("le32_straddles", self.pos))
        self._absorb(data)

    def ad(self, data: bytes, more: bool):
        self._begin_op(FLAG_A, more)
        if data and self.pos + len(data) == RATE:
            self.events.append(("message_ends_at_166", len(data)))
        self._absorb(data)

    def prf(self, n: int, more: bool) -> bytes:
        self._begin_op(FLAG_I | FLAG_A | FLAG_C, more)
        return self._squeeze(n)


class Merlin:
    def __init__(self, label: bytes = None, hashing=True, exported: bytes = None):
        if exported is not None:
            self.strobe = Strobe(hashing=hashing, exported=exported)
            return
        self.strobe = Strobe(b"Merlin v1.0", hashing)
        self.append_message(b"dom-sep", label)

    def append_message(self, label: bytes, msg: bytes):
        self.strobe.meta_ad(label, False)
        self.strobe.meta_ad(len(msg).to_bytes(4, "little"), True)
        self.strobe.ad(msg, False)

    def challenge_bytes(self, label: bytes, n: int) -> bytes:
        self.strobe.meta_ad(label, False)
        self.strobe.meta_ad(n.to_bytes(4, "little"), True)
        return self.strobe.prf(n, False)


def merlin_test_vector(protocol: bytes, label: bytes, msg: bytes, challenge_label: bytes, n: int) -> bytes:
    m = Merlin(protocol)
    m.append_message(label, msg)
    return m.challenge_bytes(challenge_label, n)


def run_program(program, data: bytes, label: bytes = None, state: bytes = None, hashing=True, max_tries=MAX_TRIES):
    """One member.  program: [(op, label, count, len)].  Returns (challenges: [32 big-endian bytes], tries: [int],
    exported state, status, the Merlin object).  With hashing=False every first draw counts as accepted.
    max_tries: draws of one challenge before the member gives up with status 1 (the library's bound is MAX_TRIES; its
    test hook TRANSCRIPT_MAX_TRIES lowers it).  As in the host twin the program stops at the first challenge that gives
    up: challenges and tries hold the accepted ones before it, and the state is unspecified."""
    assert 1 <= max_tries <= MAX_TRIES
    m = Merlin(label, hashing) if state is None else Merlin(hashing=hashing, exported=state)
    at, challenges, tries, status = 0, [], [], 0
    for op, lab, count, ln in program:
        for _ in range(count):
            if status:
                break
            if op == TR_APPEND:
                m.append_message(lab, data[at: at + ln])
                at += ln
                continue
            assert op == TR_CHALLENGES
            for t in range(1, max_tries + 1):
                dest = m.challenge_bytes(lab, 32)
                if not hashing or int.from_bytes(dest, "big") < R:       # SetBytesCanonical: equal to r is a rejection
                    m.append_message(lab, dest)                            # AppendScalars of the canonical value: the same bytes
                    challenges.append(dest)
                    tries.append(t)
                    break
                m.strobe.events.append(("rejected_draw", dest))
            else:
                status = 1
    assert at <= len(data)
    return challenges, tries, m.strobe.export(), status, m


def positions(program, label: bytes = None, start=None):
    """(pos, pos_begin, cur_flags) after the program, and the events on the way, by positions alone."""
    state = None if start is None else bytes(200) + bytes(start) + bytes(5)
    consumed = sum(c * n for op, _, c, n in program if op == TR_APPEND)
    _, _, st, _, m = run_program(program, bytes(consumed), label, state, hashing=False)
    return (st[200], st[201], st[202]), m.strobe.events, m.strobe.permutations


def consumed_bytes(program) -> int:
    return sum(c * n for op, _, c, n in program if op == TR_APPEND)


def n_challenges(program) -> int:
    return sum(c for op, _, c, _ in program if op == TR_CHALLENGES)


# ---- the programs the tests run -------------------------------------------------------------------------
def prelude_program(ell: int):
    """curdleproof.go:217-224: the 4 ell + 1 instance encodings under curdleproofs_step1, ell challenges vec_a."""
    return [(TR_APPEND, b"curdleproofs_step1", 4 * ell + 1, 48), (TR_CHALLENGES, b"curdleproofs_vec_a", ell, 0)]


PRELUDE_LABEL = b"curdleproofs"
BOUNDARY_LABEL = b"boundary"
BOUNDARY_EVENTS = ("message_ends_at_166", "header_straddles", "le32_straddles", "header_ends_at_166_no_forced_f")


def boundary_programs():
    """For each event of BOUNDARY_EVENTS the first program of a small family in which it occurs, found by replaying
    positions: a filler message of n bytes under a label of L bytes, then two messages and two challenges, then a
    message again (what follows a challenge must work too).  {event: program}."""
    found = {}
    for ev in BOUNDARY_EVENTS:
        for L in (3, 0, 32, 17):
            for n in range(0, 2 * RATE):
                prog = [(TR_APPEND, b"f" * L, 1, n), (TR_APPEND, b"msg", 2, 40), (TR_CHALLENGES, b"ch" + b"x" * (L // 2), 2, 0),
                        (TR_APPEND, b"after", 1, 7)]
                _, events, _ = positions(prog, BOUNDARY_LABEL)
                if any(e[0] == ev and (ev != "header_ends_at_166_no_forced_f" or e[1] == FLAG_I | FLAG_A | FLAG_C) for e in events):
                    found[ev] = prog
                    break
            if ev in found:
                break
    return found


# ---- the retry fixture (tests/golden/gen_transcript_retry_cases.py writes it) ----------------------------
RETRY_LABEL = b"retry fixture"
RETRY_PROGRAM = [(TR_APPEND, b"seed", 1, 32), (TR_CHALLENGES, b"c", 8, 0)]


def retry_member_data(seed: int) -> bytes:
    return hashlib.shake_256(b"transcript retry case %d" % seed).digest(32)
