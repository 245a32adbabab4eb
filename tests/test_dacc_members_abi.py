"""The member form's surface without a device: the two symbols are exported and declared, and the binding refuses
arguments that do not fit before it begins an accumulation."""
import os
import re

import numpy as np
import pytest

import dacc_members_model as MM
import dacc_model as M
from conftest import ROOT

NEW = ("curdle_dacc_run_members", "curdle_stat_dacc_members")


def test_symbols_are_exported_and_declared(cm):
    header = open(os.path.join(ROOT, "include", "curdle_msm.h")).read()
    import ctypes
    lib = ctypes.CDLL(cm.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/curdle_msm.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in cm.SYMBOLS
    assert re.search(r"#define\s+CURDLE_DACC_MAX_MEMBERS\s+(\d+)", header).group(1) == str(MM.MAX_MEMBERS)
    assert MM.MAX_MEMBERS >= 64 and MM.MAX_MEMBER_SLOTS >= 64 * (132 + 64 * 496)     # what 64 Whisk members need
    assert "CURDLE_DACC_MAX_MEMBER_SLOTS ((size_t)1 << 22)" in header and MM.MAX_MEMBER_SLOTS == 1 << 22


def test_stat_reads_without_a_device(cm):
    st = cm.stat_dacc_members()
    assert set(st) == {"runs", "members", "one_by_one"} and all(v >= 0 for v in st.values())


def test_binding_refuses_what_does_not_fit_before_it_begins(cm, oracle):
    c, cmem, xmem = MM.group_case(20, 16, 5, 1)
    base = np.zeros((257, 12), dtype=np.uint64)
    _, inst, loose = M.case_points(c, base)
    checks, pool, xs = M.pack_checks(c.checks), M.pack_fr(c.pool, oracle), M.pack_fr(c.extra_scalars, oracle)
    before = cm.stat_dacc_members()

    def call(cmem=cmem, xmem=xmem, n_members=5, xs=xs, **kw):
        return cm.dacc_run_members(None, inst, checks, cmem, n_members, pool, loose, xs, xmem, **kw)   # no base set: never reached

    for bad in (dict(cmem=cmem[:-1]), dict(cmem=cmem + [0]), dict(xmem=xmem[:-1]), dict(xmem=xmem + [0]), dict(xs=xs[:-1]),
                dict(cmem=[5] + cmem[1:]), dict(xmem=[5] + xmem[1:]), dict(cmem=[-1] + cmem[1:]), dict(n_members=0),
                dict(n_members=-1), dict(n_members=max(cmem))):
        with pytest.raises(ValueError):
            call(**bad)
    assert cm.stat_dacc_members() == before
