"""The engine as it builds by default applies range ops across a leaf block's split (MT_LEAF_SPLIT,
csrc/mt_core.h rangeLeaf) on the host emulation: a build with the -DMT_EVRANGE counters and neither
-DMT_LEAF_SPLIT nor -DMT_INSERT_LEAF on its command line, against the oracle and, pool for pool,
against the -DMT_LEAF_SPLIT=0 -DMT_INSERT_LEAF=0 build of tests/test_leaf_split.py.

Event slot 7 (range ops applied across a block split) proves the default is on.  On the generated
streams it is above zero on every document.  On the hand-built cases it equals the count each case
is built for (tests/leaf_split_cases.py RANGE_CASES): one, except for the document of client 63,
whose range op is refused by the fused step as ever and must stay at zero.
"""
import functools
import os

import pytest

from fluidframework_amd.engine import Engine
from oracle_lib import gen_params, generate
from emu_lib import DEPS, ROOT, SRC, _atomic_build
from test_emu_parity import CONFIGS, ann_props, compare
from test_range_leaf import assert_same_state, state
import leaf_split_cases as LS
import test_leaf_split as TLS


def default_lib():
    lib = os.path.join(ROOT, "tests", "emu", "libmtemu_leafsplit_default.so")
    if not os.path.exists(lib) or any(os.path.getmtime(lib) < os.path.getmtime(d) for d in DEPS):
        _atomic_build(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-DMT_G_MWMIN=64",
                       "-DMT_BPC_CHECK=1", "-DMT_EVRANGE", "-o", None, SRC], lib)
    return lib


def default_factory():
    lib = default_lib()
    return lambda n, **kw: Engine(n, lib_path=lib, prefix="emu_", **kw)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(batch, props, documents, expected slot 7 per document or None) of one named input."""
    if name in ("remove", "annotate"):
        batch, props, hits = LS.build_ranges(name)
        return batch, props, len(hits), hits
    props = ann_props()
    p = gen_params(seed=11, n_docs=4, **CONFIGS[name])
    batch, st, _ = generate(p, props)
    assert st == [0] * 4
    return batch, props, 4, None


def run(batch, props, n, factory):
    """One build on the batch, checked against the oracle; its state and events."""
    last = batch.op_offsets[1:] - 1
    eng = compare(batch, props, n, factory=factory)
    got = state(eng, n, batch.arrays["msn"][last], batch.arrays["seq"][last]), TLS.events(eng, n)
    eng.close()
    return got


@functools.lru_cache(maxsize=None)
def both_off(name):
    """The three-visit build's state and events on the input: computed once, never changed."""
    batch, props, n, _ = inputs(name)
    return run(batch, props, n, TLS.factory(0, 0))


@pytest.mark.parametrize("name", ["remove", "annotate", "cfg2", "cfg3"])
def test_default_build_applies_range_ops_across_block_splits(name):
    batch, props, n, hits = inputs(name)
    s0, ev0 = both_off(name)
    s1, ev1 = run(batch, props, n, default_factory())
    assert_same_state(s1, s0)
    assert (ev0[:, TLS.EV_RANGE_SPLIT] == 0).all()
    print(name, "range ops across a block split per document:", ev1[:, TLS.EV_RANGE_SPLIT])
    if hits is None:
        assert (ev1[:, TLS.EV_RANGE_SPLIT] > 0).all(), ev1[:, 6:9]
    else:
        for d, case in enumerate(LS.RANGE_CASES):
            assert ev1[d, TLS.EV_RANGE_SPLIT] == hits[d], f"{case}: {ev1[d, TLS.EV_RANGE_SPLIT]}, expected {hits[d]}"
    # the counters that both builds keep are unchanged: no room is counted either way
    assert (ev1[:, TLS.EV_NO_ROOM] == ev0[:, TLS.EV_NO_ROOM]).all() and (ev1[:, TLS.EV_FUSED] == ev0[:, TLS.EV_FUSED]).all()
