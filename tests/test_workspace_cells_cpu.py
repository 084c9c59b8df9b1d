"""The table of tests/workspace_cells.py against the plan report (`omgx_plan_describe`, `omgx_plan_schur_tiles`: host only, no device):
every case sits in exactly the cell the table states -- wave path, workspace mode, agents per CU, Schur-tile leaves -- and on the
wave path its LDS part lies on the stated side of `kLdsHalf`.  A change to `work_split` or `plan_for_mode` that moves a class into
another cell fails here, on a machine without a GPU, and the message says that the GPU cases then need a new representative."""
import pytest

from workspace_cells import CASES, LDS_HALF, LDS_PER_CU, WAVE_CASES, build_class, threads


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_the_plan_reports_the_cell_of_the_table(case):
    problem, P, plan = build_class(case, 1)            # (asserts the cell)
    print('%s: wave path %d, mode %d, %d B of LDS, %d per CU (%d threads), leaves %s (bw %s)'
          % (case.id, plan['wave_path'], plan['ws_mode'], plan['lds_bytes'], case.per_cu, threads(case), plan['leaf_sizes'], plan['leaf_bw']))
    assert 0 < plan['lds_bytes'] <= LDS_PER_CU
    if case.wave_path:
        assert plan['ws_mode'] in (0, 4, 5)
        assert plan['lds_bytes'] <= LDS_HALF if case.per_cu == 2 else plan['lds_bytes'] > LDS_HALF
        # the hyperplane leaves (one per obstacle, banded) are the Schur tiles; the diagonal leaf of the terminal slacks comes last
        assert plan['n_leaf'] == case.n_obs + 1 and case.schur_tiles == case.n_obs


def test_the_table_covers_every_cell_it_can():
    """Modes 0, 4, 5 with two per CU and with one per CU -- all six cells --, the headline as the control."""
    cells = sorted((c.mode, c.per_cu) for c in WAVE_CASES)
    assert cells == [(0, 1), (0, 2), (4, 1), (4, 2), (5, 1), (5, 2)]
    assert len([c for c in CASES if not c.wave_path]) == 1
