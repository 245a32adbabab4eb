"""What sharing ONE host body between the two constant-time MSM families can break (csrc/msm_ct_call.h: seg_shape,
stage_scalars, seg_walk_sum_fetch; csrc/msm_ct_api.hip, csrc/msm_ct_bases_api.hip), on the GPU: the families called one
behind the other on ONE context and ONE thread, so on one slot and its buffers.  A layout computed from the previous
call's k, a verdict or status word left by the other family (or by the single call's 160-byte layout in between) and
offsets kept from a larger call would all show as a wrong result or a wrong refusal here.  Every result is compared with
the point of the big-integer model through the C oracle (msm_ct_model.expected_jac, as the sibling files do) and, for
equal inputs, bit for bit across the forms; the counters against deltas computed from the shapes."""
import numpy as np
import pytest

import msm_ct_batch_model as bm
import msm_ct_bases_model as cb
import msm_ct_model as mm
from msm_ct_model import R

pytestmark = pytest.mark.gpu
BITS = 16
CHUNKS = (8, 16)
# k = 1, 2, 3 over segment sizes {0, 1, 2, 513}: an odd k (the table ends 8 bytes past a multiple of 16 and the row list
# follows it), an empty MSM first, in the middle and last, and a segment above the 512-term tail (one level launch)
SHAPES = ((513,), (0, 2), (2, 0), (1, 513, 2), (1, 0, 1), (2, 1, 0))
VERDICT = "a scalar is not below 2^scalar_bits"


class Env:
    """One base set of 300 points (three of them infinity) with a handle per chunk width, and a call's arrays: the pairs
    of a shape are rows wandering over the set with 16-bit scalars, the plain forms get the gathered points."""

    def __init__(self, gpu, oracle, coracle):
        self.gpu, self.o, self.co = gpu, oracle, coracle
        self.base = cb.Bases(oracle, 300, (0, 150, 299))
        self.pts = self.base.limbs(coracle)
        self.handles = {c: gpu.CtBases(self.pts, c) for c in CHUNKS}
        self._cases = {}

    def case(self, counts, start=0, bad=None):
        """(rows, pair points, scalars, offsets, expected uint64[k, 18], expected of all pairs as ONE MSM); `bad`: the
        index of a pair whose scalar is exactly 2^BITS (no expected results then)."""
        key = (tuple(counts), start, bad)
        if key not in self._cases:
            _, ks = mm._pool(self.o)
            total = sum(counts)
            rows = [(start + 13 * p) % self.base.n for p in range(total)]
            sc = [ks[(start + p) % len(ks)] & ((1 << BITS) - 1) for p in range(total)]
            if bad is not None:
                sc[bad] = 1 << BITS
            offs = np.cumsum([0] + list(counts)).astype(np.uint64)
            sums = [sum(k * self.base.g[r] for k, r in zip(sc[a:b], rows[a:b]) if self.base.g[r] is not None) % R
                    for a, b in zip(offs[:-1].astype(int), offs[1:].astype(int))]
            want = np.array([mm.expected_jac(self.o, self.co, s) for s in sums], dtype=np.uint64).reshape(-1, 18)
            r = np.array(rows, dtype=np.uint32)
            self._cases[key] = (r, np.ascontiguousarray(self.pts[r]), mm.to_limbs(self.o, sc), offs, want,
                                mm.expected_jac(self.o, self.co, sum(sums) % R))
        return self._cases[key]

    def stats(self):
        g = self.gpu
        return g.stat_msm_ct(), g.stat_msm_ct_batch(), g.stat_msm_ct_bases()

    # The six calls of the interleaving: name -> (call, the counters it moves).  Resident forms read device copies.
    def call(self, name, counts, c, **kw):
        import torch
        g, h = self.gpu, self.handles[c]
        r, pp, sc, offs, want, one = self.case(counts, **kw)
        n, k, nonempty, cbits = sum(counts), len(counts), sum(1 for v in counts if v), cb.chunks(BITS, c)
        moved = {"ct": (0, 0, 0), "batch": (0, 0, 0), "bases": (0, 0, 0)}
        if name in ("resident batch", "bases resident batch"):
            d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
            d_pp = torch.from_numpy(pp.view(np.int64)).to("cuda:0")
            torch.cuda.synchronize()
        if name == "host batch":
            got = g.msm_g1_ct_batch(pp, sc, offs, BITS)
        elif name == "resident batch":
            got = g.msm_g1_ct_batch_device(d_pp.data_ptr(), d_sc.data_ptr(), offs, BITS)
        elif name == "bases host batch":
            got = h.msm_batch(sc, offs, r, BITS)
        elif name == "bases resident batch":
            got = h.msm_batch_device(d_sc.data_ptr(), offs, r, BITS)
        elif name == "single":
            got = g.msm_g1_ct(pp, sc, BITS)
        else:
            assert name == "bases single"
            got = h.msm(sc, r, BITS)
        if name in ("host batch", "resident batch"):
            moved["ct"], moved["batch"] = (n, 1, nonempty), (1, k, bm.level_launches(counts))
        elif name in ("bases host batch", "bases resident batch"):
            moved["batch"], moved["bases"] = (1, k, cb.level_launches(counts, c, BITS)), (1, n * cbits, nonempty)
        elif name == "single":
            moved["ct"] = (n, 1, 1)
        else:
            moved["bases"] = (1, n * cbits, 1)
        return got, (one if "single" in name else want), moved


ORDER = ("host batch", "resident batch", "bases host batch", "bases resident batch", "single", "bases single")


@pytest.fixture(scope="module")
def env(gpu, oracle, coracle):
    e = Env(gpu, oracle, coracle)
    yield e
    for h in e.handles.values():
        h.free()


def _refused(gpu, call):
    with pytest.raises(gpu.CurdleError) as e:
        call()
    assert e.value.code == gpu.EINVAL and VERDICT in e.value.msg, e.value.msg


def test_the_families_interleaved_and_their_counters(env):
    """host batch, resident batch, bases host batch, bases resident batch, curdle_msm_g1_ct, the bases single call, in
    this order and in reverse, for every shape and both chunk widths: each result is the model's, equal inputs give
    identical words in every form, and over the WHOLE run the three counter sets move by what the shapes say -- per
    batch (total, 1, nonempty) and (1, k, levels), per single call (n, 1, 1) and nothing on the batch counter, the bases
    forms never on curdle_stat_msm_ct, no table built."""
    assert bm.level_launches([513]) == 1 and cb.level_launches([513], 8, BITS) == 2 and cb.level_launches([2], 8, BITS) == 0
    before = env.stats()
    total = {"ct": [0, 0, 0], "batch": [0, 0, 0], "bases": [0, 0, 0]}
    for c in CHUNKS:
        for counts in SHAPES:
            seen = {}
            for name in ORDER + ORDER[::-1]:
                got, want, moved = env.call(name, counts, c)
                assert got.shape == want.shape and (got == want).all(), (c, counts, name)
                kind = "single" if "single" in name else "batch"
                assert (seen.setdefault(kind, got) == got).all(), (c, counts, name)
                for key, d in moved.items():
                    total[key] = [a + b for a, b in zip(total[key], d)]
    after = env.stats()
    delta = [{n: after[i][n] - before[i][n] for n in after[i]} for i in range(3)]
    assert delta[0] == dict(zip(("pairs", "walks", "sums"), total["ct"])), delta[0]
    assert delta[1] == dict(zip(("calls", "msms", "levels"), total["batch"])), delta[1]
    assert delta[2] == dict(zip(("tables", "calls", "lanes", "msms"), [0] + total["bases"])), delta[2]


@pytest.mark.parametrize("c", CHUNKS)
def test_a_stale_verdict_does_not_cross_families(env, c):
    """A scalar of exactly 2^scalar_bits fails a call of one family with the documented text and counts nothing; the
    NEXT call, of the other family on the same slot with good scalars, gives the right result.  Both directions, host and
    resident forms, and once with the single call's 160-byte layout between two batched calls -- refused itself, and
    behind a refused batch."""
    gpu = env.gpu
    counts = (1, 513, 2)
    for first, then in (("host batch", "bases host batch"), ("bases host batch", "host batch"),
                        ("resident batch", "bases resident batch"), ("bases resident batch", "resident batch")):
        for bad in (0, 1 + 512, 515):
            before = env.stats()
            _refused(gpu, lambda: env.call(first, counts, c, bad=bad))
            assert env.stats() == before, (first, bad)
            got, want, _ = env.call(then, counts, c)
            assert (got == want).all(), (first, then, bad)
    # a refused batch, the single call, a batch of the other family
    for first, then in (("host batch", "bases host batch"), ("bases host batch", "host batch")):
        _refused(gpu, lambda: env.call(first, counts, c, bad=515))
        for name in ("single", then):
            got, want, _ = env.call(name, counts, c)
            assert (got == want).all(), (first, name)
        # a good batch, the single call refused, a batch of the other family
        got, want, _ = env.call(first, counts, c)
        assert (got == want).all(), first
        before = env.stats()
        _refused(gpu, lambda: env.call("single", counts, c, bad=3))
        _refused(gpu, lambda: env.call("bases single", counts, c, bad=3))
        assert env.stats() == before
        got, want, _ = env.call(then, counts, c)
        assert (got == want).all(), (first, then)


@pytest.mark.parametrize("c", CHUNKS)
def test_grow_then_shrink(env, c):
    """A batch of one 513-pair MSM, then k = 3 MSMs of one pair each, in each family and across them: offsets computed
    from the previous call's sizes would put the status word, the table or the rows elsewhere."""
    big, small = (513,), (1, 1, 1)
    for names in (("host batch", "host batch"), ("bases host batch", "bases host batch"), ("host batch", "bases resident batch"),
                  ("bases resident batch", "resident batch")):
        for name, counts, start in ((names[0], big, 0), (names[1], small, 40), (names[0], small, 40)):
            got, want, _ = env.call(name, counts, c, start=start)
            assert (got == want).all(), (names, name, counts)
