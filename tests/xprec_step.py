"""One Krylov step restated in extended precision (np.longdouble), from f64 inputs -- the yardstick of the one-launch step's envelope
tests (tests/test_gpu_fstep_envelope.py) and of their CPU pin (tests/test_xprec_step.py).

Inputs: the operator as COO triplets (rows, cols, vals), the basis V (n x m, f64, column m - 1 = v, normalised), beta (the three-term
coefficient of Lanczos).  Outputs: alpha (Lanczos) or the column h of H (Arnoldi), beta = |r|, the unnormalised new column r and the
normalised one q = r / beta, the Gram row g = V'v, and for each output the SCALE its tolerance is measured against (below).

Reference statements, KrylovKit.jl:
  lanczosrecurrence, ClassicalGramSchmidt2    src/factorizations/lanczos.jl:313-324
  lanczosrecurrence, ModifiedGramSchmidt2     src/factorizations/lanczos.jl:325-336
  arnoldirecurrence!!                         src/factorizations/arnoldi.jl:239-245
  orthogonalize!! CGS / CGS2 / MGS / MGS2     src/orthonormal.jl:378-384, 394-399, 414-423, 434-439 (reorthogonalize: 385-393, 424-433)
MGS is sequential, as in the reference.  Nothing here calls the f64 oracle (oracle/krylov_oracle.py casts to float64).

The library's low-synchronisation form of MGS (`lowsync_*`) is restated here too: rhs = p - alpha0 g, (I + L) s = rhs with L the
strictly-lower Gram matrix of V whose row m - 1 is g, coefficients s + alpha0 e_m.  It equals the sequential MGS in exact arithmetic;
its `variant` argument builds the WRONG forms the tolerance must tell apart (test_xprec_step.py):
  "cgs"       CGS coefficients in place of MGS (L = 0)
  "lagged"    the Gram row of the previous step: row m - 1 of L taken from row m - 2
  "drop"      one inner product (p_{m-1}) with the rows of one grid block left out (`drop_rows`)
  "nofold"    alpha0 not folded into the last coefficient

Tolerance (`bound`).  Every device quantity x is compared elementwise with this reference x_ref as
    |x_dev - x_ref| <= C * (m + width + 2 + ceil(log2 n)) * u * scale(x),      u = 2^-53, C = 8,
where scale(x) is the expression of x evaluated with absolute values:
  - w0 = A v - beta v_prev:  scale |A||v| + |beta||v_prev| (width fused multiply-adds per row, then one more);
  - inner products <a, b> over n rows:  scale sum |a||b| -- the device sums them in trees (row pairs per thread, wave, block, grid)
    whose depth is ceil(log2 n) plus short sequential segments, which C absorbs;
  - the coefficients s (the solve (I + L) s = rhs, rhs = p - alpha0 g):  the sum of |terms| of each, |V|'scale(w) + |alpha0| |g|
    + |L| |s| (CGS: no |L| term) -- the errors of rhs pass through (I + L)^-1, whose norm stays small for kappa(V) <= 1e2;
  - the update r = w0 - V c:  scale(w0) + |V| |c| (c = s + alpha0 e_m), m more roundings per row plus |V| times the coefficients'
    errors; a second pass repeats the last two steps with scale(r) of the first in place of scale(w0);
  - beta = |r|:  || scale(r) ||_2;   q = r / beta:  scale(r) / beta + |q| scale(beta) / beta;
  - alpha = alpha0 + s_{m-1}:  scale(alpha0) + scale(s_{m-1});  g_j = <v_j, v>:  sum |v_j||v|.
Each rounding contributes at most u times the absolute value it rounds, and no chain of dependent roundings is longer than
m (solve / update) + width (apply) + 2 (three-term part, final scale) + ceil(log2 n) (reductions): the classical gamma_K bound with
K = m + width + 2 + ceil(log2 n).  C = 8 covers the sequential segments of the reductions and the one rounding of the comparison.
The errors the test must catch (the four variants above) are larger by many orders of magnitude on the skewed bases of
`skewed_basis` (test_xprec_step.py::test_bound_discriminates)."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53
C_BOUND = 8.0


# ---- inputs shared by the CPU pin and the GPU envelope tests ------------------------------------------------------------------
def skewed_basis(n: int, m: int, seed: int, spread: float = 0.03) -> np.ndarray:
    """m unit columns whose overlaps are ~1e-2 .. 1e-1 (kappa(V) <= ~1e2): V = G (I + E), columns normalised, G Gaussian with
    orthonormal-ish columns, E strictly random with entries ~ spread"""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, m))
    if n >= m:
        G, _ = np.linalg.qr(G)
    E = spread * rng.standard_normal((m, m))
    np.fill_diagonal(E, 0.0)
    V = G @ (np.eye(m) + E)
    return V / np.linalg.norm(V, axis=0)


def ell_operator(n: int, width: int, seed: int) -> sp.csr_matrix:
    """a general ELL matrix: exactly `width` stored entries in every row (the library keeps it in the ELL format), the diagonal and
    width - 1 scattered columns (fixed distinct offsets mod n), random values"""
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], rng.choice(np.arange(1, n), size=width - 1, replace=False)])
    rows = np.repeat(np.arange(n), width)
    cols = (rows + np.tile(offs, n)) % n
    vals = rng.standard_normal(n * width)
    vals[::width] += 4.0
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, n))


def coo(A) -> tuple:
    A = sp.coo_matrix(A)
    return A.row.astype(np.int64), A.col.astype(np.int64), A.data.astype(np.float64)


def max_width(A) -> int:
    A = sp.csr_matrix(A)
    return int(np.max(np.diff(A.indptr))) if A.shape[0] else 0


# ---- extended-precision building blocks --------------------------------------------------------------------------------------
def _apply(op, x):
    rows, cols, vals = op
    y = np.zeros(len(x), dtype=LD)
    np.add.at(y, rows, vals.astype(LD) * x[cols])
    return y


def _dot(a, b):
    return np.sum(a * b, dtype=LD)


@dataclass
class Step:
    """result of one step; `scale` holds scale(x) of the module docstring for every output"""
    alpha: Optional[LD] = None           # Lanczos
    h: Optional[np.ndarray] = None       # Arnoldi: column of H (length m)
    beta: LD = LD(0)
    r: Optional[np.ndarray] = None       # unnormalised new column
    q: Optional[np.ndarray] = None       # normalised new column (r itself when beta == 0)
    g: Optional[np.ndarray] = None       # Gram row V[:, :m-1]'v
    scale: Dict[str, object] = field(default_factory=dict)


def _finish(st: Step, r, r_scale):
    st.r = r
    st.beta = np.sqrt(_dot(r, r))
    st.scale["r"] = r_scale
    st.scale["beta"] = np.sqrt(np.sum(r_scale * r_scale, dtype=LD))
    if st.beta > 0:
        st.q = r / st.beta
        st.scale["q"] = r_scale / st.beta + np.abs(st.q) * st.scale["beta"] / st.beta
    else:
        st.q = r.copy()
        st.scale["q"] = r_scale
    return st


def gram_lower(V, extended: bool = True) -> np.ndarray:
    """L[i, j] = <v_i, v_j> for j < i, 0 elsewhere; longdouble, or (extended=False) the f64 BLAS product -- its error, u |V|'|V|, is
    what the device's own Gram rows carry, far below the bound, and it is n m^2 / 2 multiply-adds faster"""
    if not extended:
        V64 = np.asarray(V, dtype=np.float64)
        return np.tril(V64.T @ V64, -1).astype(LD)
    VL = np.asarray(V, dtype=LD)
    return np.tril(VL.T @ VL, -1)


def _fsub(L, rhs):
    """(I + L) s = rhs by forward substitution"""
    s = np.array(rhs, dtype=LD)
    for i in range(1, len(rhs)):
        s[i] -= np.dot(L[i, :i], s[:i])
    return s


def _coef_scale(aV, w_scale, s, aLg=None, alpha0=LD(0), g=None):
    """sum of |terms| of each coefficient in the kernel's form: |V|'scale(w) [+ |alpha0| |g|] [+ |L| |s| (MGS family)]"""
    sig = aV.T @ w_scale
    if g is not None:
        sig = sig + abs(alpha0) * np.abs(g)
    if aLg is not None:
        sig = sig + aLg @ np.abs(s)
    return sig


def _abs_gram(VL):
    """|L| with row m - 1 = |g|: the strictly-lower Gram matrix of the whole basis (v = its last column)"""
    return np.abs(gram_lower(VL, extended=False))


# ---- the reference recurrences (sequential, as in KrylovKit.jl) ---------------------------------------------------------------
def lanczos_step(op, V, beta, orth: str) -> Step:
    """lanczosrecurrence for "cgs2" (lanczos.jl:313-324) and "mgs2" (:325-336); V = [v_1 .. v_m] (v = V[:, m-1]), beta the previous beta"""
    VL = np.asarray(V, dtype=LD)
    n, m = VL.shape
    aV = np.abs(VL)
    v, vprev = VL[:, m - 1], VL[:, m - 2]
    bL = LD(beta)
    rows, cols, vals = op
    Av = _apply(op, v)                                                  # w = apply(A, v)                               :314 / :326
    Av_scale = _apply((rows, cols, np.abs(vals)), np.abs(v))
    w0_scale = Av_scale + abs(bL) * np.abs(vprev)
    g = VL.T @ v
    st = Step()
    if orth == "cgs2":
        alpha0 = _dot(v, Av)                                            # alpha = inner(v, w)                           :315
        a_scale = _dot(np.abs(v), Av_scale)
        w = Av - bL * vprev                                             # w = add!!(w, V[end-1], -beta)                 :316
        w = w - alpha0 * v                                              # w = add!!(w, v, -alpha)                       :317
        s = VL.T @ w                                                    # w, s = orthogonalize!!(w, V, ClassicalGramSchmidt())   :318
        r = w - VL @ s
        sig = _coef_scale(aV, w0_scale, s, None, alpha0, g)
    elif orth == "mgs2":
        w = Av - bL * vprev                                             # w = add!!(w, V[end-1], -beta)                 :327
        alpha0 = _dot(v, w)                                             # w, alpha = orthogonalize!!(w, v, ModifiedGramSchmidt())   :328
        a_scale = _dot(np.abs(v), w0_scale)
        w = w - alpha0 * v
        s = np.zeros(m, dtype=LD)
        for j in range(m):                                              # for q in V: w, s = orthogonalize!!(w, q, MGS)  :330-332
            s[j] = _dot(VL[:, j], w)
            w = w - s[j] * VL[:, j]
        r = w
        sig = _coef_scale(aV, w0_scale, s, _abs_gram(VL), alpha0, g)
    else:
        raise ValueError(orth)
    st.alpha = alpha0 + s[m - 1]                                        # alpha += s[end]                               :319 / :333
    st.scale["alpha"] = a_scale + sig[m - 1]
    c = np.abs(s)
    c[m - 1] += abs(alpha0)
    st.g = g[: m - 1]
    st.scale["g"] = aV[:, : m - 1].T @ np.abs(v)
    return _finish(st, r, w0_scale + aV @ c)


def arnoldi_step(op, V, orth: str) -> Step:
    """arnoldirecurrence!! (arnoldi.jl:239-245): w = apply(A, v); r, h = orthogonalize!!(w, V, h, orth) for "cgs", "mgs", "cgs2", "mgs2"
    (orthonormal.jl:378-384, 414-423, 394-399, 434-439); beta = norm(r)"""
    VL = np.asarray(V, dtype=LD)
    n, m = VL.shape
    aV = np.abs(VL)
    v = VL[:, m - 1]
    rows, cols, vals = op
    w = _apply(op, v)
    w_scale = _apply((rows, cols, np.abs(vals)), np.abs(v))
    aLg = None if orth.startswith("cgs") else _abs_gram(VL)
    h = np.zeros(m, dtype=LD)
    h_scale = np.zeros(m, dtype=LD)
    for _ in range(2 if orth in ("cgs2", "mgs2") else 1):
        if orth.startswith("cgs"):                                      # project!! ; unproject!!   :380-383 / :387-391
            s = VL.T @ w
            w = w - VL @ s
        else:                                                           # for (i, q) in enumerate(b): s = inner(q, v); v = add!!(v, q, -s)   :416-421 / :426-431
            s = np.zeros(m, dtype=LD)
            for j in range(m):
                s[j] = _dot(VL[:, j], w)
                w = w - s[j] * VL[:, j]
        h += s
        h_scale += _coef_scale(aV, w_scale, s, aLg)
        w_scale = w_scale + aV @ np.abs(s)
    st = Step(h=h)
    st.scale["h"] = h_scale
    st.g = (VL.T @ v)[: m - 1]
    st.scale["g"] = aV[:, : m - 1].T @ np.abs(v)
    return _finish(st, w, w_scale)


def mgs_coefficients(V, x) -> tuple:
    """sequential MGS of x against the columns of V (orthonormal.jl:414-423): coefficients and their scale"""
    VL = np.asarray(V, dtype=LD)
    w = np.asarray(x, dtype=LD)
    m = VL.shape[1]
    s = np.zeros(m, dtype=LD)
    for j in range(m):
        s[j] = _dot(VL[:, j], w)
        w = w - s[j] * VL[:, j]
    return s, _coef_scale(np.abs(VL), np.abs(np.asarray(x, dtype=LD)), s, _abs_gram(VL))


# ---- the library's low-synchronisation algebra (k_lanczos_fstep, k_lanczos_coef) ---------------------------------------------
def _lowsync_pass(VL, w, L, first_g, alpha0, variant, drop_rows):
    m = VL.shape[1]
    p = VL.T @ w
    if variant == "drop":
        p[m - 1] -= _dot(VL[drop_rows, m - 1], w[drop_rows])
    rhs = p - alpha0 * first_g
    if variant == "cgs":
        s = rhs
    else:
        Lx = L.copy()
        Lx[m - 1, : m - 1] = first_g[: m - 1]
        if variant == "lagged" and m >= 3:
            Lx[m - 1, : m - 1] = 0
            Lx[m - 1, : m - 2] = L[m - 2, : m - 2]
        s = _fsub(Lx, rhs)
    return s


def lowsync_lanczos(op, V, beta, orth: str, variant: Optional[str] = None, drop_rows=None, extended_gram: bool = True) -> Step:
    """the kernel's form of lanczosrecurrence: [alpha0 | p = V'w | g = V'v] in one reduction, rhs = p - alpha0 g, (I + L) s = rhs (MGS2;
    CGS2: s = rhs), r = w - V (s + alpha0 e_m), alpha = alpha0 + s_{m-1}"""
    VL = np.asarray(V, dtype=LD)
    n, m = VL.shape
    v, vprev = VL[:, m - 1], VL[:, m - 2]
    Av = _apply(op, v)
    w = Av - LD(beta) * vprev
    alpha0 = _dot(v, Av) if orth == "cgs2" else _dot(v, w)
    g = VL.T @ v
    L = gram_lower(VL, extended_gram)
    s = _lowsync_pass(VL, w, L, g, alpha0, "cgs" if orth == "cgs2" and variant is None else variant, drop_rows)
    c = s.copy()
    if variant != "nofold":
        c[m - 1] += alpha0
    st = Step(alpha=alpha0 + s[m - 1] if variant != "nofold" else s[m - 1])
    st.g = g[: m - 1]
    return _finish(st, w - VL @ c, np.zeros(n, dtype=LD))


def lowsync_arnoldi(op, V, orth: str, variant: Optional[str] = None, drop_rows=None, extended_gram: bool = True) -> Step:
    """the kernel's form of arnoldirecurrence!!: per pass p = V'w, (I + L) s = p with row m - 1 of L = g (MGS family; CGS: s = p), w -= V s"""
    VL = np.asarray(V, dtype=LD)
    n, m = VL.shape
    v = VL[:, m - 1]
    w = _apply(op, v)
    g = VL.T @ v
    L = gram_lower(VL, extended_gram)
    h = np.zeros(m, dtype=LD)
    for _ in range(2 if orth in ("cgs2", "mgs2") else 1):
        s = _lowsync_pass(VL, w, L, g, LD(0), "cgs" if orth.startswith("cgs") and variant is None else variant, drop_rows)
        w = w - VL @ s
        h += s
    st = Step(h=h)
    st.g = g[: m - 1]
    return _finish(st, w, np.zeros(n, dtype=LD))


# ---- tolerance --------------------------------------------------------------------------------------------------------------
def bound(scale, m: int, width: int, n: int) -> np.ndarray:
    """C * (m + width + 2 + ceil(log2 n)) * u * scale -- derivation in the module docstring"""
    K = m + width + 2 + math.ceil(math.log2(max(n, 2)))
    return C_BOUND * K * U * np.asarray(scale, dtype=np.float64)


def excess(dev, ref, scale, m: int, width: int, n: int) -> float:
    """max over the elements of |dev - ref| / bound: <= 1 passes"""
    d = np.abs(np.asarray(dev, dtype=LD) - np.asarray(ref, dtype=LD)).astype(np.float64)
    b = bound(scale, m, width, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(b > 0, d / np.where(b > 0, b, 1.0), np.where(d > 0, np.inf, 0.0))
    return float(np.max(q)) if q.size else 0.0


# ---- the launcher's choice of shape (kk_launch_lanczos_fstep) ------------------------------------------------------------------
FS_MAX_BLOCKS = 128


def fstep_shape(nrows: int, threads: int, fstep_blocks: int, num_cus: int):
    """(NP, G) the launcher picks, or None when the rows do not fit (kk_fstep_capacity_rows)"""
    gmax = max(1, min(FS_MAX_BLOCKS, fstep_blocks, num_cus))
    if nrows > gmax * 8 * 256 * 2:
        return None
    chunks = -(-nrows // (threads * 2))
    np_need = -(-chunks // gmax)
    NP = 1 if np_need <= 1 else (2 if np_need <= 2 else (4 if np_need <= 4 else 8))
    G = -(-chunks // NP)
    assert np_need <= (4 if threads == 1024 else 8) and 1 <= G <= gmax
    return NP, G


def block_rows(b: int, threads: int, NP: int, n: int) -> np.ndarray:
    """the rows block b of the launch owns: row pairs ((b NP + i) threads + tid) * 2, i < NP"""
    lo = b * NP * threads * 2
    return np.arange(lo, min(lo + NP * threads * 2, n))


# ---- the inputs of the envelope tests (tests/test_gpu_fstep_envelope.py; their CPU pin: tests/test_xprec_step.py) -------------
# (threads, fstep_blocks, grid nx x ny, NP, G): every (threads, NP) the launcher can reach, G = 1, 2, 3, 5, 64, 65, 127, 128 and a few
# between, odd and even row counts, 99 x 331 = 32 769 rows = 64 x 512 + 1
ENVELOPE_SHAPES = [
    (256, 128, (20, 25), 1, 1),
    (256, 128, (21, 23), 1, 1),
    (256, 128, (31, 33), 1, 2),
    (256, 128, (36, 40), 1, 3),
    (256, 128, (50, 51), 1, 5),
    (256, 128, (180, 182), 1, 64),
    (256, 128, (99, 331), 1, 65),
    (256, 128, (254, 256), 1, 127),
    (256, 128, (255, 257), 1, 128),
    (256, 8, (70, 100), 2, 7),
    (256, 128, (300, 400), 2, 118),
    (256, 8, (120, 120), 4, 8),
    (256, 8, (173, 173), 8, 8),
    (256, 8, (128, 240), 8, 8),
    (512, 128, (40, 50), 1, 2),
    (512, 8, (100, 120), 2, 6),
    (512, 8, (128, 256), 4, 8),
    (1024, 128, (100, 100), 1, 5),
    (1024, 8, (128, 256), 2, 8),
]
ENVELOPE_M = [2, 3, 4, 5, 8, 31, 32, 33, 63, 64, 65, 66, 96, 127, 128]
ENVELOPE_ORTH = [("lanczos", "cgs2"), ("lanczos", "mgs2"), ("arnoldi", "cgs"), ("arnoldi", "mgs"), ("arnoldi", "cgs2"), ("arnoldi", "mgs2")]
LARGE_N = 100_000        # at and above: basis sizes up to 66 only (the run stays short)


def envelope_cases(shape_index: int):
    """the (kind, orth, m, operator) combinations run at one shape: every orthogonaliser once, m rotating through ENVELOPE_M so that
    every (orthogonaliser, m) pair appears at some shape, the operator rotating through the shifted 2-D Laplacian, ELL width 7 and 13
    (and, for Arnoldi, the convection-diffusion stencil)"""
    i = shape_index
    n = ENVELOPE_SHAPES[i][2][0] * ENVELOPE_SHAPES[i][2][1]
    out = []
    for o, (kind, orth) in enumerate(ENVELOPE_ORTH):
        m = ENVELOPE_M[(7 * i + 3 * o) % len(ENVELOPE_M)]
        if n >= LARGE_N:
            m = min(m, 66)
        ops = ["laplacian", "ell7", "ell13"] if kind == "lanczos" else ["convdiff", "ell7", "ell13", "laplacian"]
        out.append((kind, orth, m, ops[(i + o) % len(ops)]))
    return out


def envelope_operator(name: str, nx: int, ny: int):
    import krylov_oracle as ko   # (the matrices only)
    n = nx * ny
    if name == "laplacian":
        return ko.laplacian_2d(nx, ny, shift_diag=10 * np.linspace(0, 1, n) ** 2)
    if name == "convdiff":
        return ko.convection_diffusion_2d(nx, ny)
    return ell_operator(n, int(name[3:]), seed=n + int(name[3:]))


def envelope_inputs(shape_index: int, case_index: int):
    """(A, V, beta_old, seed) of one case: V skewed with column m - 1 the unit vector v; the device is handed r = beta_old v"""
    threads, fb, (nx, ny), NP, G = ENVELOPE_SHAPES[shape_index]
    kind, orth, m, opname = envelope_cases(shape_index)[case_index]
    seed = 1000 * shape_index + case_index
    A = envelope_operator(opname, nx, ny)
    V = skewed_basis(nx * ny, m, seed)
    beta_old = 0.75 + 0.5 * np.random.default_rng(seed).random()
    return A, V, beta_old


# ---- one expand! through the C ABI and its check (tests/test_gpu_fstep_envelope.py, tests/test_gpu_sweep_envelope.py) --------------
ORTHS = {"cgs": "ClassicalGramSchmidt", "mgs": "ModifiedGramSchmidt", "cgs2": "ClassicalGramSchmidt2", "mgs2": "ModifiedGramSchmidt2"}


def orth(kk, name):
    return getattr(kk, ORTHS[name])()


def one_step(kk, c, op, A, V, beta_old, kind, orth_name, on_step=None):
    """upload V with r = beta_old v in column m - 1, one expand! with k = m - 1; returns the device's results and its f64 inputs as read back
    (`on_step()`: called right behind the expand!, before anything else is launched)"""
    n, m = V.shape
    lib = c._lib
    B = kk.DeviceBasis(n, m + 2, c)
    for j in range(m - 1):
        B.upload(j, V[:, j])
    B.upload(m - 1, beta_old * V[:, m - 1])
    o = orth(kk, orth_name)
    b, npass = C.c_double(), C.c_int()
    if kind == "lanczos":
        a = C.c_double()
        kk._lib.check(lib.kk_lanczos_expand(op.handle, B.handle, 0, m - 1, o.code, o.eta, beta_old, C.byref(a), C.byref(b), C.byref(npass)))
        out = {"alpha": a.value}
    else:
        h = np.zeros(m)
        kk._lib.check(lib.kk_arnoldi_expand(op.handle, B.handle, 0, m - 1, o.code, o.eta, beta_old, h.ctypes.data_as(kk._lib.c_dp), C.byref(b),
                                            C.byref(npass)))
        out = {"h": h}
    if on_step is not None:
        on_step()
    out["beta"] = b.value
    Vd = np.stack([B.download(j) for j in range(m)], axis=1)     # the device's inputs: column m - 1 = v as normalised in the stream
    out["r"] = B.download(m)      # (a column stored normalised is handed out times beta: an error in the stored column shows here)
    if orth_name.startswith("mgs"):
        # the Gram row the host took (row m - 1 of the slab's cached rows) through an operation that must use it: MGS of a probe vector
        # against columns 0 .. m - 1 with the solve on the host's rows (low-sync, unfused)
        x = np.random.default_rng(m).standard_normal(n)
        B.upload(m + 1, x)
        c.set_option("fuse_passes", 0)
        out["probe"] = (x, B.orthogonalize(kk.HipVec(B, m + 1), kk.ModifiedGramSchmidt(), 0, m, want_norm=False)[0])
        c.set_option("fuse_passes", 1)
    B.free()
    return out, Vd


def check_step(out, Vd, A, beta_old, kind, orth, width):
    n, m = Vd.shape
    op = coo(A)
    ref = lanczos_step(op, Vd, beta_old, orth) if kind == "lanczos" else arnoldi_step(op, Vd, orth)
    key = "alpha" if kind == "lanczos" else "h"
    errs = {key: excess(out[key], getattr(ref, key), ref.scale[key], m, width, n),
            "beta": excess(out["beta"], ref.beta, ref.scale["beta"], m, width, n),
            "r": excess(out["r"], ref.r, ref.scale["r"], m, width, n),
            "q": excess(out["r"] / out["beta"], ref.q, ref.scale["q"], m, width, n)}
    if "probe" in out:
        x, s = out["probe"]
        s_ref, s_scale = mgs_coefficients(Vd, x)
        errs["gram"] = excess(s, s_ref, s_scale, m, 0, n)
    return errs
