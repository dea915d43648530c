"""Inserts whose split row's right half and new row enter their leaf block in one visit
(MT_INSERT_LEAF) and range ops whose right halves split their leaf block (MT_LEAF_SPLIT) on the
device: the hand-built cases of tests/leaf_split_cases.py and generated streams against the
oracle, under block residency and with every pool in HBM (the two engine instantiations the
replay kernels are built from).
"""
import pytest

from oracle_lib import gen_params, generate
from test_emu_parity import CONFIGS, ann_props, compare
from test_gpu_parity import gpu_engine
import leaf_split_cases as LS

pytestmark = pytest.mark.gpu

RESIDENCIES = [(2, 0, 0, 0), (0, 0, 0, 0)]
IDS = ["blk", "hbm"]


@pytest.mark.parametrize("res", RESIDENCIES, ids=IDS)
def test_gpu_hand_built_cases_match_oracle(res):
    batch, props, paired, _ = LS.build()
    compare(batch, props, len(paired), factory=gpu_engine, residency=res)


@pytest.mark.parametrize("res", RESIDENCIES, ids=IDS)
@pytest.mark.parametrize("mode", ["remove", "annotate"])
def test_gpu_hand_built_range_cases_match_oracle(mode, res):
    batch, props, hits = LS.build_ranges(mode)
    compare(batch, props, len(hits), factory=gpu_engine, residency=res)


@pytest.mark.parametrize("res", RESIDENCIES, ids=IDS)
@pytest.mark.parametrize("cfg", ["cfg2", "cfg3"])
def test_gpu_generated_streams_match_oracle(cfg, res):
    props = ann_props()
    p = gen_params(seed=19, n_docs=8, **CONFIGS[cfg])    # 1,500 messages per document
    batch, st, _ = generate(p, props)
    assert st == [0] * 8
    compare(batch, props, 8, factory=gpu_engine, residency=res)


@pytest.mark.parametrize("res", RESIDENCIES, ids=IDS)
def test_gpu_compaction_between_the_cut_and_the_linking(res):
    """The text arena at 2,048 units for documents that insert some 3,900 (tests/test_leaf_split.py)."""
    props = ann_props()
    p = gen_params(seed=11, n_docs=4, **CONFIGS["cfg2"])
    batch, st, _ = generate(p, props)
    assert st == [0] * 4
    compare(batch, props, 4, factory=gpu_engine, residency=res, text=2048)
