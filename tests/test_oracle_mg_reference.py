"""The fp64 multigrid reference (tests/mg_reference.py) pinned on the CPU: it equals the oracle's level operators in fp64 and
tests/golden/np_step.py's sequential restatement, and the oracle's own float arithmetic meets its fp32 bounds — so the constants K
are those of an honest float implementation, not fitted to the device."""
import os
import sys

import numpy as np
import pytest

from tests import mg_reference as mr
from tests import pipeline_checks as pc


def built(lib, dtype, n=8, levelCnt=3):
    ctx, c = pc.make_ctx(lib, n=n, dtype=dtype, levelCnt=levelCnt, coarseSolver=5)
    pc.prepare(ctx)
    ctx.update_state(ctx.get_dv())
    ctx.build_hessian()
    ctx.build_mg()
    return ctx


def all_operators(ctx, dtype, label):
    T = np.float64 if dtype == 1 else np.float32
    ref = mr.Hierarchy(ctx, 3)
    assert ref.levels[0].colour_blocks == [8] * 8  # every colour and every in-block position occur on level 0
    rep = mr.Report(label, mr.U64 if dtype == 1 else mr.U32)
    mr.check_operators(ctx, ref, T, rep, 3, jacobi_levels=(0, 1), pcg_its=(3, 10) if dtype == 1 else (), pcg_levels=(0, 2) if dtype == 1 else ())
    x = np.asarray(ctx.project(np.random.default_rng(5).standard_normal((ctx.Nn, 3))), T)
    v, m, K = ref.vcycle(x)
    rep.add("vcycle", 0, ctx.vcycle(x), v, m, K)
    return rep


def test_reference_equals_oracle_fp64(oracle):
    """n = 8 cube, three levels, GS on every level (coarseSolver 5): spmv, restrict, prolong, the Galerkin matrices, smooth kinds
    0 / 1 / 2 / 5 and the V-cycle of the oracle against the reference on the oracle's exported levels"""
    rep = all_operators(built(oracle, 1), 1, "oracle fp64")
    rep.check(normwise_tol=1e-12)
    assert len(rep.rows) > 60


@pytest.mark.parametrize("wide", [False, True], ids=["float_sums", "wide_sums"])
def test_float_oracle_within_fp32_bounds(oracle, wide):
    """K calibrated without a GPU: the oracle in float arithmetic (sums in float like the reference, or in double: oracle_lib.wide_sums)
    against the fp64 reference on the oracle's own float matrices meets |got - ref| <= K u m with u = 2^-24"""
    from tests.oracle_lib import wide_sums
    with wide_sums(wide):
        rep = all_operators(built(oracle, 0), 0, "oracle fp32" + (" wide" if wide else ""))
        rep.check()


def _ell(H, n):
    """a dense 3n x 3n matrix as padded ELL (col, column-major 3x3 val), the layout ctx.matrix() exports"""
    B = H.reshape(n, 3, n, 3).transpose(0, 2, 1, 3)  # B[i, j] = block (i, j)
    nz = np.abs(B).max((2, 3)) > 0
    k = int(nz.sum(1).max())
    col, val = np.zeros((n, k), np.int32), np.zeros((n, k, 9))
    for i in range(n):
        js = np.nonzero(nz[i])[0]
        col[i, :len(js)] = js
        col[i, len(js):] = i  # padding: zero blocks on the row's own column
        val[i, :len(js)] = B[i, js].transpose(0, 2, 1).reshape(len(js), 9)
    return col, val


def test_reference_equals_np_step():
    """the vectorised sweeps against np_step.gs_smooth (one row at a time, O(n^2)), and the two-level V-cycle with its PCG top
    against np_step.Hierarchy, on np_step.tiny_cloud"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import np_step as ns
    c = ns.tiny_cloud()
    coord = np.array(sorted(ns.touched_nodes(c)))
    st = ns.Step(c, coord)
    H = st.hessian(st.dv0)
    n = len(coord)
    lev = mr.Level(*_ell(H, n), coord)
    assert sum(b > 0 for b in lev.colour_blocks) == 8
    b = st.project(np.random.default_rng(7).standard_normal((n, 3)))
    for its in (1, 2, 3, 4):
        un, rn = ns.gs_smooth(H, st.coord, np.zeros((n, 3)), b, its)
        u, r, _, _ = lev.gs(np.zeros((n, 3)), b, its)
        assert mr.normwise(u, un) < 1e-13 and mr.normwise(r, rn) < 1e-12, (its, mr.normwise(u, un), mr.normwise(r, rn))
    hier = ns.Hierarchy(H, st.coord)
    ref = mr.Hierarchy.__new__(mr.Hierarchy)
    coord1 = np.array(hier.coord1)
    P = hier.P
    pcol = np.zeros((n, 8), np.int32)
    pw = np.zeros((n, 8))
    for i in range(n):
        js = np.nonzero(P[i])[0]
        pcol[i, :len(js)], pw[i, :len(js)] = js, P[i, js]
    ref.levels = [lev, mr.Level(*_ell(hier.A1, len(coord1)), coord1)]
    ref.transfers = [mr.Transfer(pcol, pw, len(coord1))]
    out, _, K = ref.vcycle(b, coarse_pcg=True)
    assert K is None
    assert mr.normwise(out, hier.vcycle(b)) < 1e-10
