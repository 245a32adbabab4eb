"""Writes tests/golden/transcript_retry_cases.npz: members of the retry program of tests/merlin_model.py (a fresh
transcript RETRY_LABEL, one 32-byte message made from the member's seed, eight challenges) whose draws, found by the
model, include what a batch of random members almost never shows:
  * a REJECTED and an ACCEPTED draw with top byte 0x73, the top byte of r: the compare is decided below the first byte;
  * a challenge of at least 6 tries.
Arrays: seeds (n), challenges (n x 8 x 32), tries (n x 8), kind (n: bit 0 rejected-with-0x73, bit 1 accepted-with-0x73,
bit 2 six tries or more, 0 an ordinary member).  Run from the repository root: python tests/golden/gen_transcript_retry_cases.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import merlin_model as mm  # noqa: E402

PER_KIND = 3


def main():
    have = {1: 0, 2: 0, 4: 0, 0: 0}
    rows = []
    seed = 0
    while any(have[k] < PER_KIND for k in have):
        ch, tries, _, status, m = mm.run_program(mm.RETRY_PROGRAM, mm.retry_member_data(seed), mm.RETRY_LABEL)
        assert status == 0
        kind = 0
        if any(e[0] == "rejected_draw" and e[1][0] == 0x73 for e in m.strobe.events):
            kind |= 1
        if any(c[0] == 0x73 for c in ch):
            kind |= 2
        if max(tries) >= 6:
            kind |= 4
        wanted = [b for b in (1, 2, 4) if kind & b and have[b] < PER_KIND] if kind else ([0] if have[0] < PER_KIND else [])
        if wanted:
            for b in (1, 2, 4):
                have[b] += 1 if kind & b else 0
            have[0] += 1 if kind == 0 else 0
            rows.append((seed, ch, tries, kind))
        seed += 1
    out = os.path.join(HERE, "transcript_retry_cases.npz")
    np.savez_compressed(out,
                        seeds=np.array([r[0] for r in rows], dtype=np.uint32),
                        challenges=np.array([[list(c) for c in r[1]] for r in rows], dtype=np.uint8),
                        tries=np.array([r[2] for r in rows], dtype=np.uint8),
                        kind=np.array([r[3] for r in rows], dtype=np.uint8))
    print("wrote %s: %d members from %d seeds tried, kinds %s" % (out, len(rows), seed, have))


if __name__ == "__main__":
    main()
