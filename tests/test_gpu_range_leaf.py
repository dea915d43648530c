"""Range ops applied in one visit to their leaf block (MT_RANGE_LEAF) on the device: the
hand-built cases of tests/range_leaf_cases.py and generated remove / annotate streams against
the oracle, under block residency and with every pool in HBM (the two engine instantiations
the replay kernels are built from).
"""
import pytest

from oracle_lib import gen_params, generate
from test_emu_parity import CONFIGS, ann_props, compare
from test_gpu_parity import gpu_engine
import range_leaf_cases as RL

pytestmark = pytest.mark.gpu

RESIDENCIES = [(2, 0, 0, 0), (0, 0, 0, 0)]
IDS = ["blk", "hbm"]


@pytest.mark.parametrize("res", RESIDENCIES, ids=IDS)
@pytest.mark.parametrize("mode", RL.MODES)
def test_gpu_hand_built_cases_match_oracle(mode, res):
    batch, props, hits = RL.build(mode)
    compare(batch, props, len(hits), factory=gpu_engine, residency=res)


@pytest.mark.parametrize("res", RESIDENCIES, ids=IDS)
@pytest.mark.parametrize("cfg", ["cfg2", "cfg3"])
def test_gpu_generated_streams_match_oracle(cfg, res):
    props = ann_props()
    p = gen_params(seed=17, n_docs=8, **CONFIGS[cfg])    # 1,500 messages per document
    batch, st, _ = generate(p, props)
    assert st == [0] * 8
    compare(batch, props, 8, factory=gpu_engine, residency=res)
