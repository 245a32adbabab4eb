"""The MSM plan on the CPU: a host-only probe (tests/plan_probe.cpp) links libcurdlemsm.so, calls make_plan over a grid of
calls -- up to 2^27 pairs, batches, base sets, window ranges and widths, every mode flag, and the chunks of host-buffer
calls as they are cut -- and the invariants the kernels rely on are checked on every plan."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def plans(cm, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_probe")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "plan_probe.cpp"), "-L" + PKG, "-lcurdlemsm", "-Wl,-rpath," + PKG,
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = []
    for line in out.splitlines():
        shape, *kv = line.split()
        row = {k: int(v) for k, v in (x.split("=") for x in kv)}
        row["shape"] = shape
        rows.append(row)
    return rows


def test_the_probe_covers_the_grid(plans):
    ok = [r for r in plans if r["rc"] == 0]
    assert len(ok) > 10000
    assert max(r["n"] for r in ok) == 1 << 27
    assert {(r["pipelined"], r["joined"], r["chunked"]) for r in ok} == {(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1)}
    chunks = [r for r in ok if r["shape"] == "chunk"]
    assert chunks and max(r["n"] for r in chunks) > 1 << 24
    # a call beyond 2^27 pairs is refused, not planned
    over = [r for r in plans if r["shape"] == "over"]
    assert over and all(r["rc"] != 0 for r in over)


def test_every_chunk_merges_at_one_limit(plans):
    for r in plans:
        if r["rc"] == 0 and r["chunked"]:
            assert r["max_small"] == 8, r


def test_the_large_bucket_queue_holds_every_bucket_over_the_limit(plans):
    """A bucket with more than max_small fragments holds more than (max_small - 1) * L entries: the queue must have room
    for as many such buckets as the call's entries can fill, or for every bucket slot.  (The scan drops what does not fit.)"""
    for r in plans:
        if r["rc"] != 0 or r["nw"] == 0:
            continue
        entries = r["nw"] * r["terms"]
        nbk = r["pk"] * r["psets"] * r["NB"]
        need = min(nbk, entries // ((r["max_small"] - 1) * r["L"]) + 1)
        assert r["max_large"] >= need, r


def test_joined_and_pipelined_calls_take_the_chained_scan(plans):
    """k_scan_one needs four SIMDs of one compute unit empty: only a synchronous call that is not joined takes it."""
    for r in plans:
        if r["rc"] != 0 or r["nw"] == 0 or r["L"] < 2:
            continue
        single_block = r["pk"] * r["NB"] <= 32768
        if r["joined"] or r["pipelined"]:
            assert r["fuse_scan"] == 3, r
        else:
            assert r["fuse_scan"] == (2 if single_block else 3), r
