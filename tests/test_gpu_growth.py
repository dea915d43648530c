"""Documents that outgrow their pools, on a real MI355X through libmtgpu.so: the checks of
tests/test_growth.py (relocation kernel, growth headroom test in the FULL replay kernels, the
grow-and-resume loop) against the oracle."""
import os

import pytest

import test_growth as tg
from fluidframework_amd.engine import Engine

pytestmark = pytest.mark.gpu


def gpu_engine(n, **kw):
    return Engine(n, device=0, **kw)


def test_gpu_autogrow_matches_oracle():
    tg.check_autogrow_parity(gpu_engine)


@pytest.mark.parametrize("cont", [0, 1 << 30])
@pytest.mark.parametrize("res", tg.RESIDENCIES)
def test_gpu_autogrow_under_residency_matches_oracle(res, cont):
    tg.check_autogrow_residency(gpu_engine, res, cont)


def test_gpu_autogrow_adversarial_matches_oracle():
    tg.check_autogrow_adversarial(gpu_engine)


@pytest.mark.parametrize("armed", [True, False])
def test_gpu_explicit_resize_mid_stream(armed):
    tg.check_explicit_resize(gpu_engine, armed)


def test_gpu_pool_accounting():
    from test_pool_accounting import check_pool_accounting
    check_pool_accounting(gpu_engine)


def test_gpu_capture_with_growth_matches_oracle():
    tg.check_capture_with_growth(gpu_engine)


def test_gpu_registers_with_growth_match_oracle():
    tg.check_registers_with_growth(gpu_engine)


def test_gpu_checkpoint_restore_across_growth():
    tg.check_checkpoint(gpu_engine)


def test_gpu_budget_stops_growth_consistently():
    tg.check_budget(gpu_engine)


def test_gpu_copy_text_headroom():
    tg.check_copy_text_headroom(gpu_engine)


def test_gpu_client_group_autogrow():
    tg.check_client_group(gpu_engine, n_msgs=150)


def test_gpu_node_host_autogrow():
    from js_lib import NODE, ROOT
    addon = os.path.join(ROOT, "fluidframework_amd", "js", "mtgpu.node")
    if NODE is None or not os.path.exists(addon):
        pytest.skip("node or the addon is not installed")
    tg.check_node(addon, n_msgs=150)
