"""The one-launch step (csrc/kk_kernels_fstep.hip) at every shape its launcher can pick -- (threads, row pairs per thread NP) = 256 x {1, 2, 4, 8},
512 x {1, 2, 4}, 1024 x {1, 2}; grids G = 1, 2, 3, 5, 64, 65, 127, 128; basis sizes m = 2 .. 128 (above 64 the solve's rows and the host-slot
stores belong to waves 1 .. 3; at 128 the 2 m + 1 values of the reduction exceed 256 threads) -- ONE step on a prepared slab whose basis is
skewed (overlaps ~1e-2 .. 1e-1), so that the low-sync solve's correction is of the order of the result and a wrong Gram row, a lagged one or
CGS coefficients in place of MGS ones are seen.  Called through the C ABI (kk_lanczos_expand / kk_arnoldi_expand) and compared with the
extended-precision reference of the same step (tests/xprec_step.py) evaluated on the device's own f64 inputs, within the bound derived there.
Every case asserts the shape it ran (options fstep_last_threads / _np / _blocks) and runs once more on the projection pair (fused_step = 0)
against the same bounds."""
import ctypes as C

import numpy as np
import pytest

import xprec_step as xp
from xprec_step import check_step, one_step, orth as _orth

pytestmark = pytest.mark.gpu


def _context(kk, threads, blocks):
    c = kk.Context(0)
    c.set_option("fstep_threads", threads); c.set_option("fstep_blocks", blocks)
    c.set_option("fused_step_m_limit", -1); c.set_option("fused_step_max_rows", 262144)
    c.set_option("mgs_mode", 1)       # (MGS in its low-synchronisation form at every length: the form the one launch carries)
    c.set_option("lookahead", 0)      # (one step: nothing enqueued behind it)
    return c


def _cases():
    for i, (threads, fb, (nx, ny), NP, G) in enumerate(xp.ENVELOPE_SHAPES):
        yield pytest.param(i, id=f"{threads}x{NP}-G{G}-n{nx * ny}")


@pytest.mark.parametrize("i", list(_cases()))
def test_one_step_at_every_launcher_shape(kk, i):
    threads, fb, (nx, ny), NP, G = xp.ENVELOPE_SHAPES[i]
    n = nx * ny
    c = _context(kk, threads, fb)
    try:
        assert xp.fstep_shape(n, threads, fb, int(c.get_option("num_cus"))) == (NP, G)
        bad = []
        ops = {}
        for j, (kind, orth, m, opname) in enumerate(xp.envelope_cases(i)):
            A, V, beta_old = xp.envelope_inputs(i, j)
            if opname not in ops:
                ops[opname] = kk.SparseOperator(A, c, symmetric=opname == "laplacian")
            width = xp.max_width(A)
            for fused in (1, 0):
                c.set_option("fused_step", fused)
                l0 = c.get_option("fstep_launches")
                out, Vd = one_step(kk, c, ops[opname], A, V, beta_old, kind, orth)
                launches = int(c.get_option("fstep_launches") - l0)
                if fused:
                    shape = (int(c.get_option("fstep_last_threads")), int(c.get_option("fstep_last_np")), int(c.get_option("fstep_last_blocks")))
                    assert launches == 1 and shape == (threads, NP, G), (kind, orth, m, launches, shape)
                else:
                    assert launches == 0
                errs = check_step(out, Vd, A, beta_old, kind, orth, width)
                print(f"reached threads={threads} NP={NP} G={G} m={m} {kind}-{orth} {opname} fused={fused}: "
                      + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
                if max(errs.values()) > 1.0 or not np.isfinite(out["r"]).all():
                    bad.append((kind, orth, m, opname, fused, errs))
        assert c.get_option("fstep_failures") == 0
        assert not bad, bad
    finally:
        c.close()


@pytest.mark.parametrize("threads,NP", [(512, 4), (1024, 2)])
def test_capacity_edge_and_the_unreachable_shapes(kk, ko, threads, NP):
    """at the capacity (fstep_blocks x 8 x 256 x 2 rows) 512-thread blocks take 4 row pairs per thread and 1024-thread ones 2 -- the most they
    can: 512 x 8 and 1024 x 4 are unreachable.  One row more and the launcher is not asked (the projection pair runs the step)"""
    c = _context(kk, threads, 8)
    try:
        cap = 8 * 8 * 256 * 2
        for n, expect in ((cap, 1), (cap + 1, 0)):
            A = xp.ell_operator(n, 7, seed=n)
            op = kk.SparseOperator(A, c)
            V = xp.skewed_basis(n, 5, seed=n)
            l0 = c.get_option("fstep_launches")
            out, Vd = one_step(kk, c, op, A, V, 1.5, "arnoldi", "mgs2")
            assert c.get_option("fstep_launches") - l0 == expect
            if expect:
                assert (c.get_option("fstep_last_threads"), c.get_option("fstep_last_np"), c.get_option("fstep_last_blocks")) == (threads, NP, 8)
            errs = check_step(out, Vd, A, 1.5, "arnoldi", "mgs2", 7)
            assert max(errs.values()) <= 1.0, errs
    finally:
        c.close()


@pytest.mark.parametrize("kind,orth", [("lanczos", "cgs2"), ("lanczos", "mgs2"), ("arnoldi", "cgs"), ("arnoldi", "mgs2")])
@pytest.mark.parametrize("m", [5, 66])
def test_exact_breakdown(kk, ko, kind, orth, m):
    """a diagonal operator on unit vectors: beta = 0 exactly.  The column holds w itself (zero; not stored normalised), no NaN anywhere in the
    slab, and a fresh factorization on the same context afterwards still matches the oracle"""
    import scipy.sparse as sp
    nx, ny = 36, 40
    n = nx * ny
    d = np.linspace(1.0, 2.0, n)
    A = sp.csr_matrix(sp.diags(d))
    c = _context(kk, 256, 128)
    try:
        op = kk.SparseOperator(A, c, symmetric=True)
        V = np.eye(n)[:, :m]
        l0 = c.get_option("fstep_launches")
        B = kk.DeviceBasis(n, m + 2, c)
        for j in range(m - 1):
            B.upload(j, V[:, j])
        B.upload(m - 1, 2.0 * V[:, m - 1])
        o = _orth(kk, orth)
        b, npass = C.c_double(), C.c_int()
        if kind == "lanczos":
            a = C.c_double()
            kk._lib.check(c._lib.kk_lanczos_expand(op.handle, B.handle, 0, m - 1, o.code, o.eta, 2.0, C.byref(a), C.byref(b), C.byref(npass)))
            # w = d v - 2 v_prev; the solve takes out -2 v_prev and alpha0 v exactly
            assert a.value == d[m - 1]
        else:
            h = np.zeros(m)
            kk._lib.check(c._lib.kk_arnoldi_expand(op.handle, B.handle, 0, m - 1, o.code, o.eta, 2.0, h.ctypes.data_as(kk._lib.c_dp), C.byref(b),
                                                   C.byref(npass)))
            assert h[m - 1] == d[m - 1] and not np.any(h[: m - 1])
        assert c.get_option("fstep_launches") - l0 == 1
        assert b.value == 0.0
        slab = np.stack([B.download(j) for j in range(m + 2)], axis=1)
        assert np.isfinite(slab).all()
        assert not np.any(slab[:, m])
        B.free()
        nx2, ny2 = 40, 30
        A2 = ko.laplacian_2d(nx2, ny2)
        x0 = np.random.default_rng(3).random(nx2 * ny2)
        it = kk.LanczosIterator(kk.SparseOperator(A2, c, symmetric=True), x0, kk.ModifiedGramSchmidt2(), capacity=12)
        f = kk.initialize(it)
        oit = ko.LanczosIterator(A2, x0.copy(), ko.MGS2); of = ko.lanczos_initialize(oit)
        for _ in range(8):
            f = kk.expand_(it, f); of = ko.lanczos_expand(oit, of)
        assert np.max(np.abs(np.array(f.alphas) - of.alphas) / np.abs(of.alphas)) < 1e-10
        assert np.max(np.abs(np.array(f.betas) - of.betas) / np.abs(of.betas)) < 1e-10
    finally:
        c.close()
