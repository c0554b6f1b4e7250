"""The one array-frame route behind sva_array_depth, _conf, _mb and _mixed
 on the engine: a group_start that goes back is refused by all
four entry points before any pair is read through it and before anything is
launched.  (The checks themselves: tests/test_array_args_cpu.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTED = ("census", "cost", "cost_mixed", "cost_fuse", "sgm_paths", "wta_hv", "path_sum",
           "wta_sum", "lr_check", "fuse_depth", "fuse_depth_conf")


def test_group_start_that_goes_back_is_refused_by_every_route(sva):
    """10 pairs, group_start = [0, 20, 10]: the ends pass and group 0's 20 pairs
    are within the 32-pair limit, but pairs[10..19] do not exist (the pair table
    holds exactly 10).  SVA_ERR_UNSUPPORTED, `groups of 1..32 pairs`, no kernel."""
    views = [np.zeros((20, 20), np.uint8) for _ in range(3)]
    p = sva.default_params(D=64, dir=1)
    pairs = [(0, 1 + j % 2, p, 0.05) for j in range(10)]
    gs = [0, 20, 10]
    m = sva.Multi([0], streams=1, flags=sva.SVA_MULTI_GATHER_PEER)
    calls = [lambda: m.array_depth(views, pairs, gs, 0.05, 1e-5, want_maps=True),
             lambda: m.array_depth_conf(views, pairs, gs, 0.05, 1e-5, 10, want_maps=True,
                                        want_costs=True),
             lambda: m.array_depth_mb(views, pairs, gs, 0.05, 1e-5, 10, want_maps=True,
                                      want_costs=True),
             lambda: m.array_depth_mixed(views, pairs, gs, [0.05, 0.05], 0.05, 1e-5, 10,
                                         want_maps=True, want_costs=True)]
    try:
        c0 = m.context(0, 0)
        c0.set_timing(sva.SVA_TIMING_ALL)
        c0.reset_timing()
        for i, call in enumerate(calls):
            with pytest.raises(sva.SvaError) as e:
                call()
            assert e.value.status == sva.SVA_ERR_UNSUPPORTED, i
            assert "groups of 1..32 pairs" in str(e.value), i
        assert {k: c0.kernel_time(k)[1] for k in COUNTED} == dict.fromkeys(COUNTED, 0)
    finally:
        m.close()
