"""The persistent MGS sweeps at every instantiation their launchers can pick -- k_mgs_persist (512 threads: NV 8 .. 40, 1024: NV 4 .. 20; rows
parked in LDS and spare registers, in LDS only or not at all; non-temporal or cache-allocating second read; the in-kernel apply),
k_mgs_panel (NV 4 / 8 / 16, P = 1 .. 3) and k_mgs_panel_lag (NV 4 / 6 / 8) -- on skewed bases (overlaps ~1e-2), where a stale parked row, a
missing in-panel correction or a dropped pending axpy moves the result by the overlaps times the coefficients, against the extended-precision
sweeps of tests/xprec_sweep.py within the bound derived in tests/xprec_step.py.  Each case builds its own context with G = num_cus blocks,
asserts ONE sweep launch of the shape the launcher's restatement predicts (options sweep_last_*), no timeout, and slab pad rows still zero.
(a) every instantiation: MGS, MGS2, orthonormalize MGS2 (normalised commit), MGSIR (two passes), a sub-range c0 > 0 per kernel;
(b) row-count edges of every bucket, G = 1 .. 65 and the whole chip; (c) basis sizes 1 .. 256; (d) one expand! per route and the in-kernel
apply; (e) an exact breakdown through orthogonalize / orthonormalize, and inside expand!, where the sweep kernels' zero-norm
commit guard is what keeps the column at 0."""
import ctypes as C

import numpy as np
import pytest

import xprec_step as xstep
import xprec_sweep as xs

pytestmark = pytest.mark.gpu

_HIP = []


def _hip():
    """the HIP runtime, loaded on first use (the CPU-only run collects this module too)"""
    if not _HIP:
        import os
        h = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipMemcpy.restype = C.c_int
        _HIP.append(h)
    return _HIP[0]


def _ctx(kk, route, G):
    c = kk.Context(0)
    assert c.get_option("mgs_persist") == 1, "the persistent routes are off on this device"
    G = int(c.get_option("device_cus")) if G is None else G
    c.set_option("num_cus", G)
    opts = {"panel_min_rows": 0, "persist_min_rows": 0, "fused_step": 0, "lookahead": 0, "persist_timeout_ms": 5000}
    if route[0] == "persist":
        _, threads, lds, nt = route
        opts.update(mgs_panel=0, mgs_mode=0, persist_threads=threads, persist_lds=lds, persist_nt=nt)
    else:
        _, mode, pw, lag = route
        opts.update(mgs_panel=1, mgs_mode=mode, panel_width=pw, panel_lag=lag)
    for k, v in opts.items():
        c.set_option(k, v)
    return c, G


SHAPE_KEYS = ("sweep_last_kernel", "sweep_last_nv", "sweep_last_nl", "sweep_last_nr", "sweep_last_threads", "sweep_last_nt", "sweep_last_apply")
PANEL_KEYS = ("sweep_last_kernel", "sweep_last_nv", "sweep_last_p")


def _shape(c):
    k = int(c.get_option("sweep_last_kernel"))
    return tuple(int(c.get_option(key)) for key in (SHAPE_KEYS if k == 1 else PANEL_KEYS))


def _column(B, col):
    """column `col` of the slab with its pad rows (ld of them, not n)"""
    n, ld, _, p = B.info()
    B.ctx.sync()
    buf = np.empty(ld)
    assert _hip().hipMemcpy(buf.ctypes.data, p + col * ld * 8, ld * 8, 2) == 0
    return buf


def _pads_zero(B, col):
    return not np.any(_column(B, col)[B.n:])


def _launches(c):
    return c.prof_get("k_mgs_persist")[1] + c.prof_get("k_mgs_panel")[1]


class Runner:
    """one context, one slab (basis V in columns 0 .. m - 1, w in column m), every call checked for launches, shape, timeouts and pad rows"""

    def __init__(self, kk, route, G, n, m, V):
        self.kk, self.route, self.n, self.m = kk, route, n, m
        self.c, self.G = _ctx(kk, route, G)
        self.want = xs.route_shape(route, n, self.G)
        self.B = kk.DeviceBasis(n, m + 1, self.c)
        for j in range(m):
            self.B.upload(j, V[:, j])
        self.B.length = m

    def run(self, w, alg, launches=1, normalize=False, c0=0):
        c, B = self.c, self.B
        B.upload(self.m, w)
        t0 = c.get_option("persist_timeouts")
        c.prof_reset(); c.prof_enable(1)
        f = B.orthonormalize if normalize else B.orthogonalize
        x, nrm, npass = f(B[self.m], alg, c0, self.m - c0)
        c.prof_enable(0)
        got = _launches(c)
        assert launches is None or got == launches, (alg.name, got, launches)
        self.launches = got
        assert _shape(c) == self.want, (alg.name, _shape(c), self.want)
        assert c.get_option("sweep_last_blocks") == self.G
        assert c.get_option("persist_timeouts") == t0
        assert _pads_zero(B, self.m)
        return x, nrm, npass, B.download(self.m)

    def close(self):
        self.B.free()
        self.c.close()


def _check(errs, bad, label):
    print(f"reached {label}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    if max(errs.values()) > 1.0:
        bad.append((label, errs))


def _sweep_errs(tag, ref, x, nrm, wd, normalized=False):
    e = {f"{tag}.s": xs.sweep_excess(x, ref, "total"), f"{tag}.nrm": xs.sweep_excess(nrm, ref, "nrm")}
    e[f"{tag}.q" if normalized else f"{tag}.w"] = xs.sweep_excess(wd, ref, "q" if normalized else "w")
    return e


def _c0_once():
    """one c0 > 0 sub-range per kernel: the first case (a) of each"""
    first = {}
    for i, (route, G, n, m) in enumerate(xs.cases_a()):
        first.setdefault(xs.route_shape(route, n, G)[0], i)
    return set(first.values())


def _ids(cases):
    return [pytest.param(*cs, id=f"{xs.route_shape(cs[0], cs[2], cs[1])}-G{cs[1]}-n{cs[2]}-m{cs[3]}") for cs in cases]


@pytest.mark.parametrize("route,G,n,m", _ids(xs.cases_a()))
def test_a_every_instantiation(kk, route, G, n, m):
    V, w = xs.sweep_inputs(n, m)
    ref1, ref2 = xs.mgs_sweeps(V, w, 1), xs.mgs_sweeps(V, w, 2)
    eta = xs.mgsir_eta(ref2, w)
    r = Runner(kk, route, G, n, m, V)
    bad = []
    try:
        errs = {}
        x, nrm, npass, wd = r.run(w, kk.ModifiedGramSchmidt())
        errs.update(_sweep_errs("mgs", ref1, x, nrm, wd))
        x, nrm, npass, wd = r.run(w, kk.ModifiedGramSchmidt2())
        errs.update(_sweep_errs("mgs2", ref2, x, nrm, wd))
        x, nrm, npass, wd = r.run(w, kk.ModifiedGramSchmidt2(), normalize=True)
        errs.update(_sweep_errs("onorm", ref2, x, nrm, wd, normalized=True))
        x, nrm, npass, wd = r.run(w, kk.ModifiedGramSchmidtIR(eta), launches=None)
        ir = (npass, r.launches)
        if npass == 2:
            errs.update(_sweep_errs("mgsir", ref2, x, nrm, wd))
        if xs.cases_a().index((route, G, n, m)) in _c0_once():
            refc = xs.mgs_sweeps(V[:, 2:], w, 1)
            x, nrm, npass, wd = r.run(w, kk.ModifiedGramSchmidt(), c0=2)
            errs.update(_sweep_errs("c0", refc, x, nrm, wd))
        _check(errs, bad, f"{r.want} G={r.G} n={n} m={m}")
    finally:
        r.close()
    assert not bad, bad
    assert ir == (2, 2), ir    # MGSIR: two passes, one sweep launch each


@pytest.mark.parametrize("route,G,nv", [pytest.param(r, G, nv, id=f"{r}-G{G or 'all'}-nv{nv}") for r, G, nv in xs.edges()])
def test_b_row_count_edges(kk, route, G, nv):
    """first and last nv of every bucket (xs.EDGE_FAMILIES); G = None: the whole chip, as many blocks as the device has CUs"""
    if G is None:
        c = kk.Context(0)
        G = int(c.get_option("device_cus"))
        c.close()
    n, m = xs.edge_case(route, nv, G)
    V, w = xs.sweep_inputs(n, m)
    ref1, ref2 = xs.mgs_sweeps(V, w, 1), xs.mgs_sweeps(V, w, 2)
    r = Runner(kk, route, G, n, m, V)
    bad = []
    try:
        errs = {}
        x, nrm, npass, wd = r.run(w, kk.ModifiedGramSchmidt())
        errs.update(_sweep_errs("mgs", ref1, x, nrm, wd))
        x, nrm, npass, wd = r.run(w, kk.ModifiedGramSchmidt2(), normalize=True)
        errs.update(_sweep_errs("onorm", ref2, x, nrm, wd, normalized=True))
        _check(errs, bad, f"{r.want} G={r.G} n={n} m={m}")
    finally:
        r.close()
    assert not bad, bad


@pytest.mark.parametrize("route,G,n,m", _ids(xs.cases_c()))
def test_c_basis_sizes(kk, route, G, n, m):
    V, w = xs.sweep_inputs(n, m)
    ref1, ref2 = xs.mgs_sweeps(V, w, 1), xs.mgs_sweeps(V, w, 2)
    r = Runner(kk, route, G, n, m, V)
    bad = []
    try:
        errs = {}
        x, nrm, npass, wd = r.run(w, kk.ModifiedGramSchmidt())
        errs.update(_sweep_errs("mgs", ref1, x, nrm, wd))
        x, nrm, npass, wd = r.run(w, kk.ModifiedGramSchmidt2())
        errs.update(_sweep_errs("mgs2", ref2, x, nrm, wd))
        _check(errs, bad, f"{r.want} G={r.G} n={n} m={m}")
    finally:
        r.close()
    assert not bad, bad


def _expand(kk, c, A, V, kind, orth, symmetric):
    """one expand! (xprec_step.one_step) with the sweep launches of the step itself counted and its shape read behind it"""
    op = kk.SparseOperator(A, c, symmetric=symmetric)
    seen = {}

    def on_step():
        c.prof_enable(0)
        seen["launches"] = _launches(c)
        seen["shape"] = _shape(c)
        seen["apply"] = int(c.get_option("sweep_last_apply"))
        seen["applies"] = c.get_option("persist_apply_launches")

    t0, a0 = c.get_option("persist_timeouts"), c.get_option("persist_apply_launches")
    c.prof_reset(); c.prof_enable(1)
    out, Vd = xstep.one_step(kk, c, op, A, V, 1.25, kind, orth, on_step=on_step)
    assert c.get_option("persist_timeouts") == t0
    seen["applies"] -= a0
    errs = xstep.check_step(out, Vd, A, 1.25, kind, orth, xstep.max_width(A))
    return errs, seen


@pytest.mark.parametrize("route", xs.CASES_D_ROUTES, ids=str)
def test_d_one_expand_per_route(kk, ko, route):
    """Lanczos MGS2 (w -= alpha0 v carried into the sweep: carry_q / carry_s) and Arnoldi MGS, MGS2 through expand!"""
    nx, ny = xs.CASES_D_GRID
    n = nx * ny
    A = ko.laplacian_2d(nx, ny, shift_diag=10 * np.linspace(0, 1, n) ** 2)
    V = xstep.skewed_basis(n, xs.CASES_D_M, seed=n)
    c, G = _ctx(kk, route, 1)
    bad = []
    try:
        want = xs.route_shape(route, n, G)
        for kind, orth in (("lanczos", "mgs2"), ("arnoldi", "mgs"), ("arnoldi", "mgs2")):
            errs, seen = _expand(kk, c, A, V, kind, orth, True)
            assert seen["launches"] == 1 and seen["shape"] == want, (kind, orth, seen, want)
            _check(errs, bad, f"{want} G={G} n={n} m={V.shape[1]} {kind}-{orth}")
    finally:
        c.close()
    assert not bad, bad


@pytest.mark.parametrize("grid,inside", xs.CASES_D_APPLY, ids=str)
def test_d_apply_inside_the_sweep(kk, ko, grid, inside):
    """k_mgs_persist<.., APPLY>: the Lanczos MGS2 step of a value-free Laplacian with an even line length forms w = A v - beta v_prev and alpha0
    in the sweep launch (NV 32 / 40, 512 threads, rows parked in LDS and registers); an odd line length keeps the separate apply"""
    nx, ny = grid
    n = nx * ny
    A = ko.laplacian_2d(nx, ny)
    V = xstep.skewed_basis(n, 5, seed=n)
    route = ("persist", 512, 2, 1)
    c, G = _ctx(kk, route, 1)
    c.set_option("persist_apply", 1)
    bad = []
    try:
        want = xs.route_shape(route, n, G)
        assert want[1] in (32, 40)
        errs, seen = _expand(kk, c, A, V, "lanczos", "mgs2", True)
        assert seen["launches"] == 1 and seen["shape"][:6] == want[:6], (seen, want)
        assert seen["apply"] == int(inside) and seen["applies"] == int(inside), seen
        _check(errs, bad, f"{want[:6] + (int(inside),)} G={G} n={n} m=5 lanczos-mgs2 apply={int(inside)}")
    finally:
        c.close()
    assert not bad, bad


BREAKDOWN_ROUTES = [("persist", 512, 2, 1), ("persist", 1024, 0, 0), ("panel", 2, 0, 0), ("panel", 0, 0, 0), ("panel", 2, 0, 1)]


@pytest.mark.parametrize("route", BREAKDOWN_ROUTES, ids=str)
def test_e_exact_breakdown(kk, route):
    """w in the span of a unit-vector basis: |w| = 0 exactly.  orthogonalize: x exact, w = 0, no NaN in the slab.  orthonormalize: beta = 0,
    x exact, the basis untouched, and -- as the reference's scale!!(v, inv(beta)) (orthonormal.jl:525) -- 0 * Inf in the column: the host
    rescales whatever the kernel committed, so the kernels' zero-norm guard is pinned by test_e_expand_breakdown, not here"""
    n, m = 6000, 5
    V = np.zeros((n, m))
    idx = [0, 3, 777, 4321, n - 1]
    for j, i in enumerate(idx):
        V[i, j] = 1.0
    w = np.zeros(n)
    w[idx] = [2.0, -1.5, 0.25, 3.0, -7.0]
    r = Runner(kk, route, 1, n, m, V)
    try:
        x, nrm, npass, wd = r.run(w, kk.ModifiedGramSchmidt2())
        assert nrm == 0.0 and not np.any(wd)
        np.testing.assert_array_equal(x, w[idx])
        assert np.isfinite(np.stack([r.B.download(j) for j in range(m + 1)], axis=1)).all()
        r.B.upload(m, w)
        x, nrm, npass = r.B.orthonormalize(r.B[m], kk.ModifiedGramSchmidt2(), 0, m)
        assert nrm == 0.0 and _shape(r.c) == r.want
        np.testing.assert_array_equal(x, w[idx])
        assert np.isnan(r.B.download(m)).all()
        np.testing.assert_array_equal(np.stack([r.B.download(j) for j in range(m)], axis=1), V)
    finally:
        r.close()


@pytest.mark.parametrize("speculate", [1, 0])
@pytest.mark.parametrize("kind,orth", [("lanczos", "mgs2"), ("arnoldi", "mgs"), ("arnoldi", "mgs2")])
@pytest.mark.parametrize("route", BREAKDOWN_ROUTES, ids=str)
def test_e_expand_breakdown(kk, route, kind, orth, speculate):
    """an exact breakdown inside expand!: a diagonal operator on unit vectors, beta = 0.  The step ends with ONE sweep launch that is asked
    to store r / beta (fold_scale, kk_krylov.hip); with beta = 0 the kernel's guard (rt > 0, 1 / rt finite) must leave r = 0, and nothing
    rescales it afterwards: column k + 1 is exactly 0 and columns 0 .. k + 1, pad rows included, hold no NaN.  Without speculation that is
    the whole slab; with it (the default) column k + 2 holds the next step's apply run ahead on r / beta -- A (0 Inf), as the reference's
    next apply would be -- which no factorization of length k + 1 reads"""
    import scipy.sparse as sp
    n, m = 6000, 5
    d = np.linspace(1.0, 2.0, n)
    A = sp.csr_matrix(sp.diags(d))
    c, G = _ctx(kk, route, 1)
    c.set_option("speculate", speculate)
    try:
        assert c.get_option("fold_scale") == 1
        want = xs.route_shape(route, n, G)
        op = kk.SparseOperator(A, c, symmetric=True)
        B = kk.DeviceBasis(n, m + 2, c)
        for j in range(m - 1):
            B.upload(j, np.eye(1, n, j)[0])
        B.upload(m - 1, 2.0 * np.eye(1, n, m - 1)[0])
        o = xstep.orth(kk, orth)
        b, npass = C.c_double(), C.c_int()
        t0 = c.get_option("persist_timeouts")
        c.prof_reset(); c.prof_enable(1)
        if kind == "lanczos":
            a = C.c_double()
            kk._lib.check(c._lib.kk_lanczos_expand(op.handle, B.handle, 0, m - 1, o.code, o.eta, 2.0, C.byref(a), C.byref(b), C.byref(npass)))
            assert a.value == d[m - 1]     # w = d v - 2 v_prev: alpha0 v and -2 v_prev leave exactly
        else:
            h = np.zeros(m)
            kk._lib.check(c._lib.kk_arnoldi_expand(op.handle, B.handle, 0, m - 1, o.code, o.eta, 2.0, h.ctypes.data_as(kk._lib.c_dp), C.byref(b),
                                                   C.byref(npass)))
            assert h[m - 1] == d[m - 1] and not np.any(h[: m - 1])
        c.prof_enable(0)
        assert _launches(c) == 1 and _shape(c) == want, (_launches(c), _shape(c), want)
        assert c.get_option("persist_timeouts") == t0
        assert b.value == 0.0
        slab = np.stack([_column(B, j) for j in range(m + 2 if speculate == 0 else m + 1)], axis=1)
        assert not np.any(slab[:, m])
        assert np.isfinite(slab).all()
        B.free()
    finally:
        c.close()
