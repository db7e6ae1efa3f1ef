"""CPU pin of the extended-precision sweep reference (tests/xprec_sweep.py) that the persistent sweep kernels' envelope tests
(tests/test_gpu_sweep_envelope.py) measure the device against: it restates the oracle's MGS, its bound tells the wrong forms a sweep kernel
could carry from the right one on the very inputs and shapes the GPU tests use, and its shape predictors restate the launchers."""
import numpy as np
import pytest

import xprec_step as xstep
import xprec_sweep as xs


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("m", [1, 4, 33])
def test_agrees_with_the_oracle_on_an_orthonormal_basis(ko, m):
    n = 1537
    rng = np.random.default_rng(m)
    V, _ = np.linalg.qr(rng.standard_normal((n, m)))
    w = V @ rng.standard_normal(m) * 5 + rng.standard_normal(n)
    cols = [np.ascontiguousarray(V[:, j]) for j in range(m)]
    for nsweeps, alg in ((1, ko.MGS), (2, ko.MGS2)):
        ref = xs.mgs_sweeps(V, w, nsweeps)
        wo, xo = ko.orthogonalize(w.copy(), cols, alg, np.empty(m))
        assert _rel(ref.total, xo) < 1e-14 and _rel(ref.w, wo) < 1e-14
        assert abs(float(ref.nrm) - np.linalg.norm(wo)) < 1e-14 * np.linalg.norm(wo)
        assert _rel(ref.q, wo / np.linalg.norm(wo)) < 1e-14
    # the pending axpy in front is the same as subtracting it first
    q, s = rng.standard_normal(n), 0.75
    a, b = xs.mgs_sweeps(V, w, 1, carry=(q, s)), xs.mgs_sweeps(V, w - s * q, 1)
    assert _rel(a.w, b.w) < 1e-15 and _rel(a.total, b.total) < 1e-15


PERSIST_TABLE = [   # (ld, G, threads, lds) -> (NV, NL, NR); ld = nv grid-rows at G = 1
    ((1 * 1024, 1, 512, 2), (8, 8, 0)), ((9 * 1024, 1, 512, 2), (16, 16, 0)), ((17 * 1024, 1, 512, 2), (24, 19, 5)),
    ((25 * 1024, 1, 512, 2), (32, 19, 9)), ((33 * 1024, 1, 512, 2), (40, 19, 9)), ((40 * 1024, 1, 512, 2), (40, 19, 9)),
    ((41 * 1024, 1, 512, 2), None),
    ((24 * 1024, 1, 512, 1), (24, 19, 0)), ((40 * 1024, 1, 512, 1), (40, 19, 0)), ((16 * 1024, 1, 512, 1), (16, 16, 0)),
    ((40 * 1024, 1, 512, 0), (40, 0, 0)), ((8 * 1024, 1, 512, 0), (8, 0, 0)),
    ((4 * 2048, 1, 1024, 2), (4, 4, 0)), ((5 * 2048, 1, 1024, 2), (8, 8, 0)), ((9 * 2048, 1, 1024, 2), (12, 9, 0)),
    ((13 * 2048, 1, 1024, 2), (16, 9, 0)), ((20 * 2048, 1, 1024, 2), (20, 9, 0)), ((20 * 2048, 1, 1024, 1), (20, 9, 0)),
    ((12 * 2048, 1, 1024, 0), (12, 0, 0)), ((21 * 2048, 1, 1024, 2), None),
    ((9 * 1024 * 65, 65, 512, 2), (16, 16, 0)), ((9 * 1024 * 65 + 1024, 65, 512, 2), (16, 16, 0)), ((8 * 1024 * 65 + 512, 65, 512, 2), (16, 16, 0)),
]
PANEL_TABLE = [     # (ld, G, mgs_mode, panel_width, panel_lag) -> (kernel, NV, P)
    ((4 * 1024, 1, 2, 0, 0), (2, 4, 3)), ((4 * 1024 + 512, 1, 2, 0, 0), (2, 8, 2)), ((8 * 1024, 1, 2, 0, 0), (2, 8, 2)),
    ((8 * 1024 + 512, 1, 2, 0, 0), (2, 16, 1)), ((16 * 1024, 1, 2, 0, 0), (2, 16, 1)), ((16 * 1024 + 512, 1, 2, 0, 0), None),
    ((4 * 1024, 1, 0, 0, 0), (2, 4, 1)), ((8 * 1024, 1, 0, 3, 1), (2, 8, 1)), ((4 * 1024, 1, 2, 2, 0), (2, 4, 2)), ((4 * 1024, 1, 2, 1, 0), (2, 4, 1)),
    ((8 * 1024, 1, 2, 3, 0), (2, 8, 2)), ((8 * 1024, 1, 2, 1, 0), (2, 8, 1)), ((16 * 1024, 1, 2, 3, 0), (2, 16, 1)),
    # lag cuts: nvl = ceil(ld / (G 896))
    ((4 * 896, 1, 2, 0, 1), (3, 4, 2)), ((4 * 896 + 1, 1, 2, 0, 1), (3, 6, 2)), ((6 * 896, 1, 2, 0, 1), (3, 6, 2)),
    ((6 * 896 + 1, 1, 2, 0, 1), (3, 8, 2)), ((8 * 896, 1, 2, 2, 1), (3, 8, 2)), ((8 * 896 + 1, 1, 2, 0, 1), (2, 8, 2)),
    ((4 * 896, 1, 2, 1, 1), (2, 4, 1)), ((4 * 896, 1, 0, 0, 1), (2, 4, 1)),
]


def test_shape_predictors_reproduce_the_launchers_table():
    for args, want in PERSIST_TABLE:
        assert xs.persist_shape(*args) == want, args
    for args, want in PANEL_TABLE:
        assert xs.panel_shape(*args) == want, args
    assert [xs.slab_ld(n) for n in (1, 512, 513, 1024, 1025, 1537, 2048)] == [512, 512, 1536, 1536, 1536, 2560, 2560]
    inst = xs.instantiations()
    assert len([i for i in inst if i[0] == 1]) == 48 and len([i for i in inst if i[0] == 2]) == 6 and len([i for i in inst if i[0] == 3]) == 3
    assert {i for i in inst if i[0] == 1 and i[6]} == {(1, 32, 19, 9, 512, 1, 1), (1, 40, 19, 9, 512, 1, 1)}


def test_gpu_cases_cover_every_instantiation():
    """the GPU cases reach every instantiation but the in-kernel apply ones (case d), whatever the route's shape is at the case's G"""
    reached = {xs.route_shape(r, n, G) for r, G, n, m in xs.cases_a()}
    assert reached == {i for i in xs.instantiations() if not (i[0] == 1 and i[6])}
    for r, G, n, m in xs.cases_b(256) + xs.cases_c():
        assert xs.route_shape(r, n, G) in reached
    # the row-count edges: every bucket reached at its first and last nv, whole-chip edges on any CU count the device may report
    for all_cus in (256, 240, 304):
        for route, G, nv in xs.edges():
            G = all_cus if G is None else G
            n, m = xs.edge_case(route, nv, G)
            assert -(-xs.slab_ld(n) // (G * xs.route_span(route))) == nv and n % 512
            assert xs.route_shape(route, n, G) in reached


def _variants(route, shape, nsweeps):
    v = ["tail_dropped", "block_missing"]
    if shape[0] == 1 and shape[2] + shape[3] > 0:
        v.append("stale_parked")
    if shape[0] != 1 and shape[2] >= 2:
        v.append("panel_cgs")
    if nsweeps == 2:
        v.append("restart_from_input")
    return v


def _discrimination_cases():
    for r, G, n, m in xs.cases_a() + [c for c in xs.cases_b(256) if c[2] <= 200_000] + [c for c in xs.cases_c() if c[3] in (2, 3, 65, 129)]:
        yield pytest.param(r, G, n, m, id=f"{r[0]}{r[1:]}-G{G}-n{n}-m{m}")


@pytest.mark.parametrize("route,G,n,m", list(_discrimination_cases()))
def test_bound_discriminates(route, G, n, m):
    """on the GPU cases' own inputs and shapes every wrong form exceeds the bound by at least 1e3 in the coefficients or the work vector,
    while the f64 restatement of the right one sits inside it"""
    V, w = xs.sweep_inputs(n, m)
    shape = xs.route_shape(route, n, G)
    P = shape[2] if shape[0] != 1 else 1
    for nsweeps in (1, 2):
        ref = xs.mgs_sweeps(V, w, nsweeps)

        def worst(out):
            S, x = out
            return max(xs.sweep_excess(S, ref, "s"), xs.sweep_excess(x, ref, "w"))

        assert worst(xs.sweeps_variant(V, w, nsweeps, "none", route, G)) < 1.0
        for variant in _variants(route, shape, nsweeps):
            if variant == "panel_cgs" and m < 2:
                continue
            assert worst(xs.sweeps_variant(V, w, nsweeps, variant, route, G, P=P)) > 1e3, variant


@pytest.mark.parametrize("route", xs.CASES_D_ROUTES, ids=str)
def test_bound_discriminates_the_dropped_carry(ko, route):
    """the Lanczos step's pending w -= alpha0 v (case d): left out, the sweep's coefficients leave the bound"""
    nx, ny = xs.CASES_D_GRID
    A = ko.laplacian_2d(nx, ny, shift_diag=10 * np.linspace(0, 1, nx * ny) ** 2)
    V = xstep.skewed_basis(nx * ny, xs.CASES_D_M, seed=nx * ny)
    w0, carry = xs.lanczos_carry(A, V, 1.25)
    ref = xs.mgs_sweeps(V, w0, 1, carry=carry)
    S, x = xs.sweeps_variant(V, w0, 1, "none", route, 1, carry=carry)
    assert xs.sweep_excess(S, ref, "s") < 1.0 and xs.sweep_excess(x, ref, "w") < 1.0
    S, x = xs.sweeps_variant(V, w0, 1, "carry_dropped", route, 1, carry=carry)
    assert xs.sweep_excess(S, ref, "s") > 1e3


def test_mgsir_pass_count_is_unambiguous_on_the_gpu_inputs():
    """case (a) runs MGSIR with an eta between the two pass ratios of its input (xs.mgsir_eta): each must leave room on both sides"""
    for route, G, n, m in xs.cases_a():
        V, w = xs.sweep_inputs(n, m)
        xs.mgsir_eta(xs.mgs_sweeps(V, w, 2), w)
