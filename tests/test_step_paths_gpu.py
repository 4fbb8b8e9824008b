"""The six newer steps behind the sort on the MI355X (run with -m gpu): every call of tests/golden/make_step_path_golden.py replayed
against what it launched and returned at the commit before their host code was given one level pass, one frame pass and one tile
fold (tests/golden/step_path_kernels.json).  The older five families have test_window_gpu.test_window_paths_launch_what_they_launched."""
import importlib.util
import os

import pytest

from sdqlpy_amd import abi
from test_window_gpu import _probed_table, hip_engine      # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_step_paths_launch_what_they_launched(hip_engine):
    """sdqh_table_window_exclude, _grouping_sets, _group_distinct, _group_moments, _sessions and _window_moments: every recorded call
    (wrapped, count-only, a capacity below the count; with and without exclusions, dense ranks, fold trees, an AVG, level_rows, columns;
    per row and per session; at the sizes where the sort, the tile scans and the upper tree levels change path) returns the code, the
    *out_n, the level counts and bit for bit the arrays it returned at the parent of the refactor, and launches exactly the kernels it
    launched there, in that order."""
    mod = importlib.util.spec_from_file_location("make_step_path_golden", os.path.join(GOLDEN_DIR, "make_step_path_golden.py"))
    recorder = importlib.util.module_from_spec(mod)
    mod.loader.exec_module(recorder)
    golden = recorder.load_golden(os.path.join(GOLDEN_DIR, "step_path_kernels.json"))
    ctx = hip_engine.ctx
    S, tile, _ = ctx.sort_geometry()
    assert golden["geometry"] == [S, tile] == [1024, 512]
    ctx.set_profiling(1)
    try:
        got = recorder.run_cases(ctx, abi, _probed_table)
    finally:
        ctx.set_profiling(0)
    assert sorted(got["calls"]) == sorted(golden["calls"]) and len(golden["calls"]) == 6 * 2 * 41
    for case, want in golden["calls"].items():
        assert got["calls"][case] == want, case
        assert set(want) >= {"rc", "n", "kernels", "sha"}, case                 # (a shrunken record compares nothing)
    for kernel in ("k_wrg_upper", "k_wmo_upper", "k_wex_ties", "k_gs_avg", "k_gd_finish", "k_mo_center", "k_ss_sessions", "k_ss_rows"):
        assert any(kernel in c["kernels"].split() for c in golden["calls"].values()), kernel
    # every call that was given arrays and succeeded has digests, every level call its level counts: no digest was dropped
    assert all(c["sha"] for name, c in golden["calls"].items() if c["rc"] == abi.OK and "count only" not in name)
    assert all("level_rows" in c for name, c in golden["calls"].items() if ("grouping_sets" in name or "group_moments" in name) and "no level_rows" not in name)
