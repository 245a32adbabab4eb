"""The MSM from 2^23 to 2^27 pairs -- the top of the supported range -- bit-exact against the closed form of the
known-discrete-log walk (tests/walk_reference.py), in every call form: device-resident, host buffers in chunks,
pipelined, window ranges, batches, without the GLV split, and with skewed scalars that fill the large-bucket queue.
And the queue's overflow: a call whose buckets over the merge limit do not fit the queue fails (knob MAX_LARGE, a test
hook that caps the queue), and the slot's next call is exact again.

The range has code paths of its own: the one-pass scatter only (the two-pass form's entries hold 24-bit term indices,
two terms per pair: refused above 2^23 pairs), the clamped accumulate-lane length, the merge limit of the load rule and
of chunks, host chunks of more than 2^24 pairs, 2^29 entries without the split.

Every case first checks that the card and the host have the memory it needs (measured on one MI355X: _NEED) and skips
with the reason if not; the library's workspaces are released between cases (curdle_shutdown)."""
import os
import resource
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_msm_gpu import rand_scalars
from walk_reference import mont_sums, walk_expected

pytestmark = pytest.mark.gpu

N_MAX = 1 << 27
GB = 1 << 30
# Bytes a case needs, measured on one MI355X (device: what the case held at its end -- the library's workspaces only grow
# within a call, so that is their peak -- and host: growth of the peak resident size), rounded up by about a tenth.  The
# module itself holds the walk's 2^27 points and scalars on the device (17.2 GB) and the scalars on the host (peak 6.7 GB
# with their generation); the host-buffer cases share one host copy of 2^26 points (6.4 GB), made by the first of them.
# Measured: 2^23 4.3 GB; 2^24 7.3; 2^25 + 3 14.6; 2^26 28.1; 2^27 55.1; host buffers 2^26 38.4, 48 x 2^20 in two chunks 28.7,
# 2^25 + 5 in three 19.3, 2^25 without folding 20.3; two pipelined 2^26 calls 56.1; the 2 x 2^26 batch 55.1; 2^25 without
# the split 19.1; the skewed 2^25 families 15.6 and 14.6 (+1.0 GB of host memory); the overflow cases 1.0.
_MODULE = (18 * GB, 8 * GB)
_DEVICE = {1 << 23: 5, 1 << 24: 8, (1 << 24) + 1: 8, (1 << 25) + 3: 16, 1 << 26: 31, 1 << 27: 61}
_NEED = {
    "host_2^26": (42 * GB, 8 * GB),
    "host_48x2^20": (32 * GB, 8 * GB),
    "host_2^25": (23 * GB, 8 * GB),
    "pipelined": (62 * GB, 1 * GB),
    "batch": (61 * GB, 1 * GB),
    "any_curve_point": (21 * GB, 1 * GB),
    "skewed": (17 * GB, 2 * GB),
    "overflow": (2 * GB, 1 * GB),
}
_NEED.update({f"device_{n}": (gb * GB, 1 * GB) for n, gb in _DEVICE.items()})


def _host_available():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


def _need(name, walk=None):
    """Skip (with the reason) when the card or the host does not have what case `name` needs right now (a host-buffer
    case whose points the module has copied already needs no more host memory for them)."""
    import torch
    dev, host = _NEED[name]
    if name.startswith("host") and walk is not None and walk.has_pts_host():
        host = 1 * GB
    free = torch.cuda.mem_get_info()[0]
    if free < dev:
        pytest.skip(f"{name}: needs {dev / GB:.0f} GB of free device memory, {free / GB:.1f} GB free")
    avail = _host_available()
    if avail < host:
        pytest.skip(f"{name}: needs {host / GB:.0f} GB of free host memory, {avail / GB:.1f} GB available")


@pytest.fixture(autouse=True)
def _fresh_context(gpu):
    """Every case starts and ends on a fresh context: the workspaces a case grew are released before the next one
    measures what is free.  Prints what the case held on the device at its end (workspaces included) and the
    process's peak resident size."""
    import torch
    gpu.shutdown()
    gpu.init(0)
    before = torch.cuda.mem_get_info()[0]
    yield
    torch.cuda.synchronize()
    held = before - torch.cuda.mem_get_info()[0]
    peak = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    print(f"[memory] {os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]}: device {held / GB:.1f} GB held at the end, "
          f"host peak rss {peak / GB:.1f} GB", file=sys.stderr)
    for knob in ("SCATTER", "HOST_CHUNKS", "HOST_FOLD", "MAX_LARGE"):
        gpu.plan_override(knob, None)
    gpu.profile_enable(False)
    gpu.shutdown()
    gpu.init(0)


class Walk:
    """The walk's 2^27 points on the device, one set of 2^27 uniform scalars on the host and on the device, and the
    closed form of any slice of them: the Montgomery sums of every aligned block of 2^20 scalars are taken once."""
    BLOCK = 1 << 20

    def __init__(self, gpu, oracle, coracle):
        import torch
        self.gpu, self.oracle, self.coracle = gpu, oracle, coracle
        self.k, self.q = oracle.Rand(27).get_frs(2)
        self.d_pts = torch.empty((N_MAX, 12), dtype=torch.int64, device="cuda:0")
        gpu.synth_points_walk_device(self.k, self.q, N_MAX, self.d_pts.data_ptr())
        head = self.d_pts[:64].cpu().numpy().view(np.uint64)
        assert (head == coracle.points_walk(self.k, self.q, 64)).all()
        self.sc = np.empty((N_MAX, 4), dtype=np.uint64)
        rng = np.random.default_rng(27)
        for lo in range(0, N_MAX, 1 << 24):                                   # (bounded temporaries)
            self.sc[lo:lo + (1 << 24)] = rand_scalars(rng, 1 << 24, oracle)
        self.d_sc = torch.from_numpy(self.sc.view(np.int64)).to("cuda:0")
        self.blocks = [mont_sums(self.sc[lo:lo + self.BLOCK]) for lo in range(0, N_MAX, self.BLOCK)]
        self._pts_host = None

    def pts(self, lo=0):
        return self.d_pts.data_ptr() + 96 * lo

    def scs(self, lo=0):
        return self.d_sc.data_ptr() + 32 * lo

    def has_pts_host(self):
        return self._pts_host is not None

    def pts_host(self, n):
        """The first n points in host memory (one copy of 2^26 points, shared by the host-buffer cases)."""
        assert n <= 1 << 26
        if self._pts_host is None:
            self._pts_host = self.d_pts[: 1 << 26].cpu().numpy().view(np.uint64)
        return self._pts_host[:n]

    def expected(self, lo, n):
        """The MSM of pairs [lo, lo + n) of the walk and of the module's scalars."""
        B, hi = self.BLOCK, lo + n
        m0 = m1 = 0
        at = lo
        while at < hi:
            end = min(hi, (at // B + 1) * B)
            if at % B == 0 and end - at == B:
                b0, b1 = self.blocks[at // B]
            else:
                b0, b1 = mont_sums(self.sc[at:end])
            m0 += b0
            m1 += b1 + (at - lo) * b0
            at = end
        o = self.oracle
        e = ((self.k + lo * self.q) * (m0 * o.R_FR_INV) + self.q * (m1 * o.R_FR_INV)) % o.R
        aff = self.coracle.scalar_mul_gen(e)
        return np.array(o.jac_to_mont_limbs(o.affine_from_mont_limbs([int(v) for v in aff])), dtype=np.uint64)

    def expected_for(self, sc, lo=0):
        """The MSM of the walk's pairs [lo, lo + len(sc)) with other scalars."""
        return walk_expected(self.oracle, self.coracle, self.k, self.q, sc, lo)


@pytest.fixture(scope="module")
def walk(gpu, oracle, coracle):
    import torch
    if torch.cuda.mem_get_info()[0] < _MODULE[0] or _host_available() < _MODULE[1]:
        pytest.skip(f"the module's inputs need {_MODULE[0] / GB:.0f} GB of device and {_MODULE[1] / GB:.0f} GB of host memory")
    w = Walk(gpu, oracle, coracle)
    yield w
    del w
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def plan_of(cm, tmp_path_factory):
    """The plan make_plan gives one single-MSM call, read with tests/plan_probe.cpp (host only)."""
    exe = str(tmp_path_factory.mktemp("plan") / "plan_probe")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "plan_probe.cpp"), "-L" + PKG, "-lcurdlemsm", "-Wl,-rpath," + PKG,
                           "-o", exe])

    def plan(n, glv=True, pipelined=False, chunked=False, c=0):
        out = subprocess.run([exe, str(n), str(int(glv)), str(int(pipelined)), str(int(chunked)), str(c)], capture_output=True,
                             text=True, check=True).stdout.splitlines()
        row = {k: int(v) for k, v in (x.split("=") for x in out[0].split()[1:])}
        row["windows"] = [tuple(int(v) for v in x.split(":")) for x in out[1].split()[1:]]  # (bits, buckets)
        return row
    return plan


# ------------------------------------------------------------------------------------------- device-resident ---
@pytest.mark.timeout(300)
def test_two_pass_scatter_at_its_last_size(gpu, walk, plan_of):
    """2^23 pairs is the largest call the two-pass scatter takes (2^24 terms of 24-bit indices); one pair more takes
    the one-pass form.  At 2^23 both forms, forced, give the same bits as the closed form."""
    n = 1 << 23
    _need(f"device_{n}")
    assert plan_of(n)["two_level"] == 1 and plan_of(n + 1)["two_level"] == 0
    exp = walk.expected(0, n)
    for scatter in (None, 1, 2):
        gpu.plan_override("SCATTER", scatter)
        assert (gpu.msm_g1_device(walk.pts(), walk.scs(), n) == exp).all(), scatter
    gpu.plan_override("SCATTER", None)
    assert (gpu.msm_g1_device(walk.pts(), walk.scs(), n + 1) == walk.expected(0, n + 1)).all()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [1 << 24, (1 << 24) + 1, (1 << 25) + 3, 1 << 26, 1 << 27])
def test_device_call(gpu, walk, plan_of, n):
    _need(f"device_{n}")
    p = plan_of(n)
    assert p["two_level"] == 0
    if n == 1 << 27:
        assert p["L"] > 128                       # the lane length clamped to at most 2^22 lanes
    got = gpu.msm_g1_device(walk.pts(), walk.scs(), n)
    assert (got == walk.expected(0, n)).all()
    if n == 1 << 24:
        gpu.plan_override("SCATTER", 2)           # asks for the two-pass form, which 2^25 terms cannot take: the same bits
        assert (gpu.msm_g1_device(walk.pts(), walk.scs(), n) == got).all()


# ---------------------------------------------------------------------------------------------- host buffers ---
@pytest.mark.timeout(300)
def test_host_call_default_chunks(gpu, walk):
    _need("host_2^26", walk)
    n = 1 << 26
    assert (gpu.msm_g1(walk.pts_host(n), walk.sc[:n]) == walk.expected(0, n)).all()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n,chunks,fold", [(48 << 20, 2, None), ((1 << 25) + 5, 3, None), (1 << 25, None, 0)])
def test_host_call_chunks(gpu, walk, plan_of, n, chunks, fold):
    """48 x 2^20 pairs in two chunks of 24 x 2^20: the regime of the chunk merge limit (a chunk's queue must be sized for
    the limit of 8 every chunk merges at, not for its own size's limit); graded chunks with a short last one; the
    reduction walking every chunk's fragments (HOST_FOLD=0)."""
    _need("host_48x2^20" if chunks == 2 else "host_2^25", walk)
    if chunks == 2:
        p = plan_of(n // 2, chunked=True, c=16)
        assert p["max_small"] == 8 and p["max_large"] == p["NB"]
    gpu.plan_override("HOST_CHUNKS", chunks)
    gpu.plan_override("HOST_FOLD", fold)
    assert (gpu.msm_g1(walk.pts_host(n), walk.sc[:n]) == walk.expected(0, n)).all()


# ---------------------------------------------------------------------------------------- pipelined, ranges ---
@pytest.mark.timeout(300)
def test_pipelined_calls_and_window_ranges(gpu, walk):
    """Two 2^26-pair calls in flight on different scalars; then the two window ranges [0, 4) and [4, W) of the pipelined
    plan, as two ranks of the window split issue them, sum (g1_sum) to the full call."""
    _need("pipelined")
    n = 1 << 26
    t0 = gpu.msm_g1_device_submit(walk.pts(), walk.scs(0), n)
    t1 = gpu.msm_g1_device_submit(walk.pts(), walk.scs(n), n)
    r1, r0 = gpu.msm_wait(t1), gpu.msm_wait(t0)
    assert (r0 == walk.expected(0, n)).all()
    assert (r1 == walk.expected_for(walk.sc[n:2 * n])).all()
    W = gpu.num_windows(n)
    assert W > 4
    ta = gpu.msm_g1_device_submit(walk.pts(), walk.scs(0), n, 0, 0, 4)
    tb = gpu.msm_g1_device_submit(walk.pts(), walk.scs(0), n, 0, 4, W)
    parts = np.stack([gpu.msm_wait(ta), gpu.msm_wait(tb)])
    assert (gpu.g1_sum(parts) == r0).all()


@pytest.mark.timeout(300)
def test_batch_of_two_2_26_msms(gpu, walk):
    """2^27 pairs in one batch: member j reads pairs [j 2^26, (j + 1) 2^26) of the walk and of the scalars."""
    _need("batch")
    n = 1 << 26
    out = gpu.msm_g1_batch_device(walk.pts(), walk.scs(), [0, n, 2 * n])
    assert (out[0] == walk.expected(0, n)).all()
    assert (out[1] == walk.expected(n, n)).all()


# ------------------------------------------------------------------------------------------- without the split ---
@pytest.mark.timeout(300)
def test_any_curve_point_at_2_25(gpu, walk, plan_of):
    """CURDLE_MSM_ANY_CURVE_POINT: 16 windows of 255-bit scalars, 2^29 entries."""
    _need("any_curve_point")
    n = 1 << 25
    assert plan_of(n, glv=False)["nw"] == 16 == gpu.num_windows(n, 0, gpu.MSM_ANY_CURVE_POINT)
    got = gpu.msm_g1_device(walk.pts(), walk.scs(), n, flags=gpu.MSM_ANY_CURVE_POINT)
    assert (got == walk.expected(0, n)).all()


# ------------------------------------------------------------------------------------------------ skewed scalars ---
@pytest.mark.timeout(300)
def test_a_few_hundred_distinct_scalars_at_2_25(gpu, walk, oracle):
    """Buckets of ~10^5 entries: every one goes through k_merge_large's chunks."""
    _need("skewed")
    import torch
    n = 1 << 25
    rng = np.random.default_rng(300)
    table = rand_scalars(rng, 300, oracle)
    sc = table[rng.integers(0, len(table), n)]
    d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
    gpu.profile_enable(1)
    assert (gpu.msm_g1_device(walk.pts(), d_sc.data_ptr(), n) == walk.expected_for(sc)).all()
    assert gpu.profile_last()["large_buckets"] > 0


def _just_over_the_limit(oracle, plan, n, rng):
    """n scalars whose GLV halves (k1, k2) have, in every window below the top, digits from 2 T distinct bucket values, each
    value taken by n / T terms -- (max_small L + 1) or a few more, which no placement of the lanes cuts into max_small
    fragments or fewer: every occupied bucket goes to the large-bucket queue, and the queue fills close to its bound.
    The top window's digits are kept below 2^13, so that s = k1 + k2 lambda stays below (r - 1) / 2 and below the split's
    rounding point: the kernels' split gives back exactly (k1, k2) (checked with the host restatement of tests/test_abi.py)."""
    from test_abi import GLV_LAMBDA, glv_split
    L, ms, wins = plan["L"], plan["max_small"], plan["windows"]
    T = n // (ms * L + 1)
    assert 2 * T <= min(b for _, b in wins[:-1])
    k1 = np.zeros(T, dtype=object)
    k2 = np.zeros(T, dtype=object)
    shift = 0
    for w, (bits, _) in enumerate(wins):
        if w + 1 < len(wins):
            vals = rng.permutation(1 << (bits - 1))[: 2 * T] + 1      # signed window: 1 .. 2^(bits-1), no carry
        else:
            vals = rng.integers(1, 1 << 13, 2 * T)
        k1 += np.array([int(v) << shift for v in vals[:T]], dtype=object)
        k2 += np.array([int(v) << shift for v in vals[T:]], dtype=object)
        shift += bits
    table = []
    for a, b in zip(k1, k2):
        s = int(a) + int(b) * GLV_LAMBDA
        assert s <= (oracle.R - 1) // 2 and glv_split(s, oracle.R) == (a, b)
        table.append(oracle.fr_to_mont_limbs(s))
    table = np.array(table, dtype=np.uint64)
    idx = rng.permutation(n) % T                                       # every table entry n // T or n // T + 1 times
    return np.ascontiguousarray(table[idx])


@pytest.mark.timeout(300)
def test_queue_filled_close_to_its_bound_at_2_25(gpu, walk, oracle, plan_of):
    """Every occupied bucket holds just over max_small fragments: the queue holds at least half of its planned capacity
    (the profile's large_buckets, read after the call) and the result is exact."""
    _need("skewed")
    import torch
    n = 1 << 25
    plan = plan_of(n)
    sc = _just_over_the_limit(oracle, plan, n, np.random.default_rng(25))
    d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
    gpu.profile_enable(1)
    assert (gpu.msm_g1_device(walk.pts(), d_sc.data_ptr(), n) == walk.expected_for(sc)).all()
    queued = gpu.profile_last()["large_buckets"]
    assert plan["max_large"] // 2 <= queued <= plan["max_large"], (queued, plan["max_large"])


# ------------------------------------------------------------------------------------- a queue that overflows ---
def _overflow_inputs(gpu, oracle, coracle, n, distinct, seed):
    import torch
    k, q = oracle.Rand(seed).get_frs(2)
    d_pts = torch.empty((2 * n, 12), dtype=torch.int64, device="cuda:0")
    gpu.synth_points_walk_device(k, q, 2 * n, d_pts.data_ptr())
    rng = np.random.default_rng(seed)
    table = rand_scalars(rng, distinct, oracle)
    sc = np.ascontiguousarray(table[rng.integers(0, distinct, 2 * n)])
    d_sc = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
    exp = [walk_expected(oracle, coracle, k, q, sc[:n]), walk_expected(oracle, coracle, k, q, sc[n:], n)]
    return d_pts, d_sc, sc, exp


@pytest.mark.timeout(300)
def test_an_overflowing_queue_fails_every_call_form(gpu, oracle, coracle):
    """With the queue capped below what the scalars queue (MAX_LARGE), the synchronous device call, the pipelined
    submit / wait, the batch and the chunked host-buffer call fail -- instead of returning a sum that reads every dropped
    bucket as one merged fragment.  Then, on the same context and slots, the same calls uncapped are exact again (the
    state a failed call may leave -- ccur, the scan chain, the merge counters -- is cleared), and a cap of exactly what
    the call queues is enough."""
    _need("overflow")
    n = 1 << 16
    d_pts, d_sc, sc, exp = _overflow_inputs(gpu, oracle, coracle, n, 300, 16)
    m = (1 << 19) + 5
    h_pts, _, h_sc, h_exp = _overflow_inputs(gpu, oracle, coracle, m, 700, 19)
    h_pts = h_pts[:m].cpu().numpy().view(np.uint64)
    h_sc = h_sc[:m]
    # the batch: 20 distinct values, so that its buckets are far over its own merge limit
    b_pts, b_sc, _, b_exp = _overflow_inputs(gpu, oracle, coracle, n, 20, 17)

    def calls():
        yield "device", lambda: gpu.msm_g1_device(d_pts.data_ptr(), d_sc.data_ptr(), n), exp[0]
        yield "pipelined", lambda: gpu.msm_wait(gpu.msm_g1_device_submit(d_pts.data_ptr() + 96 * n, d_sc.data_ptr() + 32 * n, n)), exp[1]
        yield "batch", lambda: gpu.msm_g1_batch_device(b_pts.data_ptr(), b_sc.data_ptr(), [0, n, 2 * n]), np.stack(b_exp)
        yield "host", lambda: gpu.msm_g1(h_pts, h_sc), h_exp[0]

    gpu.profile_enable(1)
    assert (gpu.msm_g1_device(d_pts.data_ptr(), d_sc.data_ptr(), n) == exp[0]).all()
    queued = gpu.profile_last()["large_buckets"]
    assert queued > 1
    gpu.profile_enable(False)
    for rnd in range(2):
        gpu.plan_override("MAX_LARGE", 1)
        for name, call, _ in calls():
            with pytest.raises(gpu.CurdleError, match="large-bucket queue overflowed"):
                call()
        gpu.plan_override("MAX_LARGE", None)
        for name, call, want in calls():
            assert (call() == want).all(), (rnd, name)
    gpu.plan_override("MAX_LARGE", queued)
    assert (gpu.msm_g1_device(d_pts.data_ptr(), d_sc.data_ptr(), n) == exp[0]).all()
    gpu.plan_override("MAX_LARGE", queued - 1)
    with pytest.raises(gpu.CurdleError, match="large-bucket queue overflowed"):
        gpu.msm_g1_device(d_pts.data_ptr(), d_sc.data_ptr(), n)
    gpu.plan_override("MAX_LARGE", None)
    assert (gpu.msm_g1_device(d_pts.data_ptr(), d_sc.data_ptr(), n) == exp[0]).all()
