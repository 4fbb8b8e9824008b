"""Edge values on the HIP library (run with -m gpu) against the exact reference of tests/edge_cases.py, with the default options
and again with the large-scan instances forced onto small inputs (`feature_min_rows` 0, a 1 KiB coarse filter): narrow twins,
dictionary codes, integer widths chosen from column ranges, code-space comparisons and the f64 atomics into LDS and HBM meet
NaN, +-inf, -0.0, subnormal values, INT64_MIN and ranges on the 24- / 32-bit boundaries.  Single-row groups are also compared
bit for bit with the CPU implementation."""
import pytest

import edge_cases as E
from sdqlpy_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_engine(hip_lib):
    eng = engine.Engine(hip_lib.context(device=0))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def oracle_engine(oracle_lib):
    import os
    eng = engine.Engine(oracle_lib.context(threads=min(16, os.cpu_count() or 1)))
    yield eng
    eng.close()


def _under(eng, options, run):
    for k, v in options.items():
        eng.ctx.set_option(k, v)
    eng.clear()
    try:
        return run()
    finally:
        for k, v in E.DEFAULT_OPTIONS.items():
            eng.ctx.set_option(k, v)
        eng.clear()


def _same_bits_as_cpu(got, want):
    assert len(got.records) == len(want.records)
    n = 0
    for (what, m, g, zeros), (what_w, m_w, w, _) in zip(got.records, want.records):
        assert what == what_w and m == m_w, (what, what_w)
        if m == 1 or zeros:
            assert E.bits(g) == E.bits(w), "%s: HIP %s, CPU %s" % (what, g.hex(), w.hex())
            n += 1
    return n


@pytest.mark.parametrize("options", ["default", "large-scan instances"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_edge_programs(hip_engine, oracle_engine, seed, options):
    opts = E.LARGE_SCAN_OPTIONS if options == "large-scan instances" else E.DEFAULT_OPTIONS
    before = hip_engine.ctx.jit_stats()
    got = _under(hip_engine, opts, lambda: [E.program_case(hip_engine.ctx, n, seed * 1000 + n) for n in E.SIZES])
    print("jit (compiled, from cache) before %s after %s" % (before, hip_engine.ctx.jit_stats()))
    want = [E.program_case(oracle_engine.ctx, n, seed * 1000 + n) for n in E.SIZES]
    assert sum(_same_bits_as_cpu(g, w) for g, w in zip(got, want)) > 100


@pytest.mark.parametrize("options", ["default", "large-scan instances"])
def test_edge_tuple_shapes(hip_engine, oracle_engine, options):
    opts = E.LARGE_SCAN_OPTIONS if options == "large-scan instances" else E.DEFAULT_OPTIONS
    got = _under(hip_engine, opts, lambda: [E.shape_case(hip_engine.ctx, n, 500 + n) for n in E.SIZES])
    want = [E.shape_case(oracle_engine.ctx, n, 500 + n) for n in E.SIZES]
    assert sum(_same_bits_as_cpu(g, w) for g, w in zip(got, want)) > 1000


@pytest.mark.parametrize("options", ["default", "large-scan instances"])
def test_edge_changed_contents(hip_engine, options):
    opts = E.LARGE_SCAN_OPTIONS if options == "large-scan instances" else E.DEFAULT_OPTIONS
    assert _under(hip_engine, opts, lambda: E.changed_contents_case(hip_engine.ctx)).checks == 6
