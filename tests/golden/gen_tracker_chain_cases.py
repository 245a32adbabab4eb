"""Writes tests/golden/tracker_chain_cases.npz: honest Whisk tracker proofs, made by this project's own prover
(cm.whisk_generate_tracker_proof), chosen for the branch the joint GLV chain of k_tracker_check takes on them.

A candidate is (k, r, seed): the tracker (rG, k rG), kComm = k G and the proof from cm.Rand(seed).  Its scalars are
recovered -- s from the proof bytes, c = (b - s) / k with b the blinder (the proof's first draw), or, for k = 0,
from the transcript (tests/merlin_model.py after tracker_api.hip member_scalars) -- split by the HOST build of the
kernels' split (curdle_selftest_op operation 11) and run through tests/glv_chain_model.py.  Per class the first
PER_CLASS members found are kept (every candidate has a seed of its own), within BUDGET candidates:

  1  `equal` at the c-table site                       4  `opposite` at the s-table site
  2  `opposite` at the c-table site, a set bit later   5  `equal` or `opposite` at bit 0
  3  `equal` at the s-table site                       6  class 1 or 2 with r = 0 (rG = krG = infinity)
                                                       7  k = 0: the c table only ever adds infinity

Arrays, one row per member: cls, k, r (32 big-endian bytes), seed, tracker, kcomm, proof, bit, site (0 s, 1 c),
step (1 equal, 2 opposite, 3 adds-infinity); and per class 1..7: tried (candidates examined until the class was full
or the budget ran out) and found.  The file is written with fixed zip dates: a second run gives the same bytes.
Run from the repository root: python tests/golden/gen_tracker_chain_cases.py"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle", "py"), os.path.join(ROOT, "go-curdleproofs_amd"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import glv_chain_model as M  # noqa: E402
import merlin_model as mm  # noqa: E402

OUT = os.path.join(HERE, "tracker_chain_cases.npz")
BUDGET = 20_000
PER_CLASS = 2
CLASSES = (1, 2, 3, 4, 5, 6, 7)
CHUNK = 500
R = M.R
KS = [k for k in M.TRACKER_KS if k]
RS = [5, 7, R - 3, 0x1F2E3D4C5B6A79880796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF % R]
STEP_CODE = {M.EQUAL: 1, M.OPPOSITE: 2, M.ADDS_INF: 3}
SITE_CODE = {M.SITE_S: 0, M.SITE_C: 1}
FIRST_SEED = {"main": 1_000, "r=0": 100_000, "k=0": 200_000}


def candidate(stream, n):
    """(k, r, seed) of candidate n of a stream: classes 1..5 share `main`, class 6 has r = 0, class 7 k = 0."""
    seed = FIRST_SEED[stream] + n
    if stream == "main":
        return KS[n % len(KS)], RS[(n // len(KS)) % len(RS)], seed
    if stream == "r=0":
        return (1, R - 1, 2, R - 2)[n % 4], 0, seed
    return 0, RS[n % len(RS)], seed


def transcript_challenge(tracker, kcomm, proof, gen):
    """tracker_api.hip member_scalars: kG, G, krG, rG, A, B under tracker_opening_proof, then the challenge."""
    data = kcomm + gen + tracker[48:] + tracker[:48] + proof[:96]
    program = [(mm.TR_APPEND, b"tracker_opening_proof", 6, 48), (mm.TR_CHALLENGES, b"tracker_opening_proof_challenge", 1, 0)]
    ch, _, _, status, _ = mm.run_program(program, data, b"whisk_opening_proof")
    assert status == 0
    return int.from_bytes(ch[0], "big")


def member_scalars(oracle, member, k, seed):
    """(s, c, b) of an honest member."""
    tracker, kcomm, proof = member
    b = oracle.Rand(seed).get_fr()
    s = int.from_bytes(proof[96:], "big")
    if k % R:
        c = (b - s) * pow(k, -1, R) % R
    else:
        c = transcript_challenge(tracker, kcomm, proof, oracle.compress(oracle.G1))
    return s, c, b


def classes_of(events, k, r):
    """{class: (bit, site, step)} of one member's trace (chain 0; chain 1 shares it unless r = 0)."""
    steps = [e for e in events if e[0] >= 0]
    got = {}

    def first(pred):
        return next((e for e in steps if pred(e)), None)

    eq_c = first(lambda e: e[1] == M.SITE_C and e[2] == M.EQUAL)
    op_c = next((e for i, e in enumerate(steps) if e[1] == M.SITE_C and e[2] == M.OPPOSITE and i + 1 < len(steps)), None)
    if k % R == 0:
        c_steps = [e for e in steps if e[1] == M.SITE_C]
        if c_steps and all(e[2] == M.ADDS_INF for e in c_steps) and not M.exceptional(steps):
            got[7] = c_steps[0]
        return got
    if r % R == 0:
        if eq_c or op_c:
            got[6] = eq_c or op_c
        return got
    if eq_c:
        got[1] = eq_c
    if op_c:
        got[2] = op_c
    for cls, kind in ((3, M.EQUAL), (4, M.OPPOSITE)):
        e = first(lambda e: e[1] == M.SITE_S and e[2] == kind)
        if e:
            got[cls] = e
    e = first(lambda e: e[0] == 0 and e[2] in (M.EQUAL, M.OPPOSITE))
    if e:
        got[5] = e
    return got


class Maker:
    """Honest members of (k, r, seed); the points of a (k, r) pair are computed once."""

    def __init__(self, cm, oracle):
        self.cm, self.oracle, self.points = cm, oracle, {}

    def member(self, k, r, seed):
        o = self.oracle
        if (k, r) not in self.points:
            rG = o.scalar_mul(r % R, o.G1)
            self.points[(k, r)] = (o.compress(rG) + o.compress(o.scalar_mul(k % R, rG)), o.compress(o.scalar_mul(k % R, o.G1)))
        tracker, kcomm = self.points[(k, r)]
        limbs = np.array(o.fr_to_mont_limbs(k % R), dtype=np.uint64)
        return tracker, kcomm, self.cm.whisk_generate_tracker_proof(tracker, limbs, self.cm.Rand(seed))


def trace_of(cm, oracle, member, k, r, seed, on_device=False):
    """The model's trace of chain 0 of a member, over the split of the given build."""
    s, c, b = member_scalars(oracle, member, k, seed)
    ss, cs = M.splits(cm, [s, c], on_device)
    return M.joint_chain(ss, cs, k, t=b)[0]


def search(cm, oracle, budget=BUDGET, log=None):
    """rows [(cls, k, r, seed, member, bit, site, step)], tried {cls: n}, found {cls: n}."""
    maker = Maker(cm, oracle)
    rows, tried, found = [], {c: 0 for c in CLASSES}, {c: 0 for c in CLASSES}
    for stream, classes in (("main", (1, 2, 3, 4, 5)), ("r=0", (6,)), ("k=0", (7,))):
        n = 0
        while n < budget and any(found[c] < PER_CLASS for c in classes):
            cands = [candidate(stream, j) for j in range(n, min(n + CHUNK, budget))]
            members = [maker.member(*cand) for cand in cands]
            scal = [member_scalars(oracle, m, cand[0], cand[2]) for m, cand in zip(members, cands)]
            sp = M.splits(cm, [v for s, c, _ in scal for v in (s, c)], False)
            for j, ((k, r, seed), m, (s, c, b)) in enumerate(zip(cands, members, scal)):
                open_classes = [c for c in classes if found[c] < PER_CLASS]
                if not open_classes:
                    break
                for c in open_classes:
                    tried[c] += 1
                events, u = M.joint_chain(sp[2 * j], sp[2 * j + 1], k, t=b)
                assert u == b and events[-1][2] in (M.OPPOSITE, M.ADDS_INF), "an honest member ends on T"
                for cls, (bit, site, step) in sorted(classes_of(events, k, r).items()):
                    if cls in open_classes:
                        found[cls] += 1
                        rows.append((cls, k, r, seed, m, bit, site, step))
            n += len(cands)
            if log:
                log("%s: %d candidates, found %s" % (stream, n, {c: found[c] for c in classes}))
    rows.sort(key=lambda row: (row[0], row[3]))
    return rows, tried, found


def arrays(rows, tried, found):
    b32 = lambda v: list((v % R).to_bytes(32, "big"))  # noqa: E731
    u8 = lambda col: np.array(col, dtype=np.uint8)  # noqa: E731
    return {
        "cls": u8([row[0] for row in rows]),
        "k": u8([b32(row[1]) for row in rows]),
        "r": u8([b32(row[2]) for row in rows]),
        "seed": np.array([row[3] for row in rows], dtype=np.uint32),
        "tracker": u8([list(row[4][0]) for row in rows]),
        "kcomm": u8([list(row[4][1]) for row in rows]),
        "proof": u8([list(row[4][2]) for row in rows]),
        "bit": np.array([row[5] for row in rows], dtype=np.int16),
        "site": u8([SITE_CODE[row[6]] for row in rows]),
        "step": u8([STEP_CODE[row[7]] for row in rows]),
        "tried": np.array([tried[c] for c in CLASSES], dtype=np.uint32),
        "found": np.array([found[c] for c in CLASSES], dtype=np.uint32),
    }


def npz_bytes(arrs):
    """An .npz whose bytes depend on the arrays alone (np.savez stamps every entry with the time of day)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrs):
            entry = io.BytesIO()
            np.lib.format.write_array(entry, np.ascontiguousarray(arrs[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), entry.getvalue())
    return buf.getvalue()


def load(path=OUT):
    """[{cls, k, r, seed, member, bit, site, step}], tried {cls: n}, found {cls: n} from the committed file."""
    z = np.load(path)
    site = {v: s for s, v in SITE_CODE.items()}
    step = {v: s for s, v in STEP_CODE.items()}
    rows = []
    for i in range(len(z["cls"])):
        rows.append({"cls": int(z["cls"][i]), "k": int.from_bytes(z["k"][i].tobytes(), "big"),
                     "r": int.from_bytes(z["r"][i].tobytes(), "big"), "seed": int(z["seed"][i]),
                     "member": (z["tracker"][i].tobytes(), z["kcomm"][i].tobytes(), z["proof"][i].tobytes()),
                     "bit": int(z["bit"][i]), "site": site[int(z["site"][i])], "step": step[int(z["step"][i])]})
    return (rows, {c: int(z["tried"][j]) for j, c in enumerate(CLASSES)},
            {c: int(z["found"][j]) for j, c in enumerate(CLASSES)})


def main():
    import bls12381_ref as oracle
    import curdlemsm as cm
    rows, tried, found = search(cm, oracle, log=print)
    data = npz_bytes(arrays(rows, tried, found))
    with open(OUT, "wb") as f:
        f.write(data)
    print("wrote %s: %d bytes, %d members" % (OUT, len(data), len(rows)))
    for c in CLASSES:
        print("class %d: %d found, %d candidates tried" % (c, found[c], tried[c]))


if __name__ == "__main__":
    main()
