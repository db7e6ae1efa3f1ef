"""CPU pin of the extended-precision single-step reference (tests/xprec_step.py) that the one-launch step's envelope tests
(tests/test_gpu_fstep_envelope.py) measure the device against: it restates the oracle's recurrences, the library's low-synchronisation
algebra equals its sequential MGS, and its tolerance tells the wrong algebras a kernel could carry from the right one on the very
inputs the GPU tests use."""
import numpy as np
import pytest

import xprec_step as xp


def _cols(V):
    return [np.ascontiguousarray(V[:, j]) for j in range(V.shape[1])]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("m", [2, 5, 33])
def test_agrees_with_the_oracle_on_an_orthonormal_basis(ko, m):
    nx, ny = 23, 19
    n = nx * ny
    A = ko.laplacian_2d(nx, ny, shift_diag=np.linspace(0, 3, n))
    op = xp.coo(A)
    V, _ = np.linalg.qr(np.random.default_rng(m).standard_normal((n, m)))
    beta = 0.8125
    for orth, ref in (("cgs2", ko.CGS2), ("mgs2", ko.MGS2)):
        st = xp.lanczos_step(op, V, beta, orth)
        w, alpha, b = ko.lanczosrecurrence(A, _cols(V), beta, ref)
        assert abs(float(st.alpha) - alpha) < 1e-14 * abs(alpha)
        assert abs(float(st.beta) - b) < 1e-14 * b and _rel(st.r, w) < 1e-14
    for orth, ref in (("cgs", ko.CGS), ("mgs", ko.MGS), ("cgs2", ko.CGS2), ("mgs2", ko.MGS2)):
        st = xp.arnoldi_step(op, V, orth)
        r, h = ko.orthogonalize(A @ V[:, m - 1], _cols(V), ref, np.empty(m))
        assert _rel(st.h, h) < 1e-14 and _rel(st.r, r) < 1e-14
        assert abs(float(st.beta) - ko.norm(r)) < 1e-14 * ko.norm(r)
    s, _ = xp.mgs_coefficients(V, V @ np.arange(1.0, m + 1))
    assert _rel(s, np.arange(1.0, m + 1)) < 1e-14


@pytest.mark.parametrize("m", [2, 3, 8, 65, 128])
def test_lowsync_algebra_is_the_sequential_mgs_on_a_skewed_basis(m):
    """rhs = p - alpha0 g, (I + L) s = rhs with row m - 1 of L = g, coefficients s + alpha0 e_m: the sequential MGS to ~1e-16 in longdouble"""
    n = 1440
    A = xp.ell_operator(n, 7, seed=m)
    op = xp.coo(A)
    V = xp.skewed_basis(n, m, seed=m)
    G = V.T @ V - np.eye(m)
    assert m == 2 or 1e-2 < np.max(np.abs(G)) < 2e-1
    assert np.linalg.cond(V) < 1e2
    seq = xp.lanczos_step(op, V, 1.25, "mgs2")
    ls = xp.lowsync_lanczos(op, V, 1.25, "mgs2")
    assert abs(ls.alpha - seq.alpha) <= 1e-16 * seq.scale["alpha"]
    assert np.max(np.abs(ls.r - seq.r)) <= 1e-16 * np.max(seq.scale["r"])
    for orth in ("mgs", "mgs2"):
        seq = xp.arnoldi_step(op, V, orth)
        ls = xp.lowsync_arnoldi(op, V, orth)
        assert np.max(np.abs(ls.h - seq.h)) <= 1e-16 * np.max(seq.scale["h"])
        assert np.max(np.abs(ls.r - seq.r)) <= 1e-16 * np.max(seq.scale["r"])
    # (CGS: the same algebra with L = 0)
    for orth in ("cgs", "cgs2"):
        seq, ls = xp.arnoldi_step(op, V, orth), xp.lowsync_arnoldi(op, V, orth)
        assert np.max(np.abs(ls.r - seq.r)) <= 1e-16 * np.max(seq.scale["r"])
    seq, ls = xp.lanczos_step(op, V, 1.25, "cgs2"), xp.lowsync_lanczos(op, V, 1.25, "cgs2")
    assert np.max(np.abs(ls.r - seq.r)) <= 1e-16 * np.max(seq.scale["r"])


def test_launcher_shapes_of_the_envelope_and_the_unreachable_ones():
    """the shapes the envelope tests ask for are the ones the launcher's rule picks (the GPU tests assert the launch itself), and by the
    capacity rule (kk_fstep_capacity_rows: blocks x 8 x 256 x 2 rows) 512 x 8 and 1024 x 4 are never picked"""
    for threads, fb, (nx, ny), NP, G in xp.ENVELOPE_SHAPES:
        assert xp.fstep_shape(nx * ny, threads, fb, 256) == (NP, G)
    reached = set()
    for fb in (8, 9, 16, 33, 64, 100, 127, 128):
        cap = fb * 8 * 256 * 2
        assert xp.fstep_shape(cap + 1, 256, fb, 256) is None
        for n in list(range(1, cap + 1, 97)) + [cap]:
            for threads in (256, 512, 1024):
                reached.add((threads, xp.fstep_shape(n, threads, fb, 256)[0]))
    assert reached == {(256, 1), (256, 2), (256, 4), (256, 8), (512, 1), (512, 2), (512, 4), (1024, 1), (1024, 2)}
    assert {(s[0], s[3]) for s in xp.ENVELOPE_SHAPES} == reached


def _discrimination_inputs():
    for i, (threads, fb, (nx, ny), NP, G) in enumerate(xp.ENVELOPE_SHAPES):
        if nx * ny > xp.LARGE_N:
            continue
        for j, (kind, orth, m, opname) in enumerate(xp.envelope_cases(i)):
            if m >= 2:
                yield pytest.param(i, j, id=f"{threads}x{NP}-G{G}-{kind}-{orth}-m{m}-{opname}")


@pytest.mark.parametrize("i,j", list(_discrimination_inputs()))
def test_bound_discriminates(i, j):
    """on the skewed inputs of the envelope tests, each wrong algebra exceeds the bound, the right one (longdouble) sits far inside it:
    (a) CGS coefficients in place of MGS, (b) the previous step's Gram row, (c) one inner product without the rows of one grid block
    (the last block of the G the case runs at), (d) alpha0 not folded into the last coefficient"""
    threads, fb, (nx, ny), NP, G = xp.ENVELOPE_SHAPES[i]
    kind, orth, m, opname = xp.envelope_cases(i)[j]
    A, V, beta_old = xp.envelope_inputs(i, j)
    n = nx * ny
    op, width = xp.coo(A), xp.max_width(A)
    drop = xp.block_rows(G - 1, threads, NP, n)
    if kind == "lanczos":
        ref = xp.lanczos_step(op, V, beta_old, orth)
        run = lambda variant: xp.lowsync_lanczos(op, V, beta_old, orth, variant, drop, n * m * m < 5e7)   # noqa: E731
        key = "alpha"
    else:
        ref = xp.arnoldi_step(op, V, orth)
        run = lambda variant: xp.lowsync_arnoldi(op, V, orth, variant, drop, n * m * m < 5e7)   # noqa: E731
        key = "h"

    def worst(st):
        return max(xp.excess(getattr(st, key), getattr(ref, key), ref.scale[key], m, width, n), xp.excess(st.r, ref.r, ref.scale["r"], m, width, n))

    assert worst(run(None)) < 1e-2
    variants = ["drop"] + (["nofold"] if kind == "lanczos" else []) + (["cgs", "lagged"] if orth.startswith("mgs") and m >= 2 else [])
    for variant in variants:
        if variant == "lagged" and m < 3:
            continue   # (m = 2: the previous step's row is empty -- the CGS case)
        assert worst(run(variant)) > 1.0, variant
