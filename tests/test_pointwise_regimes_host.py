"""Host side of tests/test_gpu_pointwise_loops.py, test_gpu_loss_kernels.py and test_gpu_reduce_adam.py (no GPU):
every size those modules use is in the launch regime it claims — the unrolled loop runs, the grid is capped, the
grid-stride loop wraps, the slab splits into ragged chunks — by the launchers' rules restated from the exported
queries. A launcher whose grid rule changes fails here first, before a GPU test silently returns to one pixel per
thread."""
import pytest

from tests import test_gpu_loss_kernels as LK
from tests import test_gpu_pointwise_loops as PL


@pytest.mark.parametrize("gcap", [3, 1])
@pytest.mark.parametrize("c", [64, 128, 256, 512])
@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_apply_unrolled_loop_runs(form, c, gcap):
    PL.regime_apply(form, c, gcap)


def test_default_apply_grid_never_unrolls_forms_1_to_3():
    """What the small grid is for: at the default cap and the other tests' m, forms 1 to 3 never enter the
    unrolled loop and form 0 does at C = 512 only."""
    for form in range(4):
        for c in (64, 128, 256, 512):
            pl, grid, u = PL.apply_plan(PL.APPLY_M, c, form, PL.APPLY_GRID)
            assert (PL.APPLY_M > (u - 1) * grid * pl) == (form == 0 and c == 512)


def test_heads_regimes():
    PL.regime_heads_fwd()
    PL.regime_heads_planes()
    PL.regime_apply_planes()
    for m in PL.APPLY_HEADS_MS:
        assert PL.regime_apply_heads(m) == PL.APPLY_HEADS_REGIMES[m]


def test_pool_regimes():
    for shape in PL.POOL_BWD_SHAPES:
        PL.regime_pool_bwd(*shape)
    PL.regime_pool_fwd()


def test_loss_regimes():
    for p in LK.P_LIST + [n * hw for n, _, hw in LK.CE_SHAPES] + [LK.P_A, LK.P_B]:
        LK.regime(p)
    rows, chunk = LK.regime(LK.P_LIST[-1])
    assert (rows, chunk) == (1024, 4101)
    assert [LK.regime(p)[0] for p in LK.P_LIST] == [1, 1, 1, 2, 4, 1024]
