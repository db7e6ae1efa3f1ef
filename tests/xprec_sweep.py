"""The persistent MGS sweeps (k_mgs_persist, k_mgs_panel, k_mgs_panel_lag) restated in extended precision, with the launchers' choice of
shape and the wrong forms a sweep kernel could carry -- the yardstick of tests/test_gpu_sweep_envelope.py and of its CPU pin
tests/test_xprec_sweeps.py.  Shares the inputs, the scale form and the bound of tests/xprec_step.py.

Reference (`mgs_sweeps`): an optional pending w -= s_c q_c, then `nsweeps` sequential MGS sweeps  for q in V: s = <q, w>; w -= s q
(src/orthonormal.jl:414-423, MGS2 :434-439, MGSIR :440-452), in np.longdouble from f64 inputs.  Every output carries the sum of the absolute
values of its terms (`scale`): a coefficient of a sweep |V|'scale(w_in) + (|V|'|V|, strictly lower) |s| (the rounding of every earlier
axpy of the sweep reaches it through |v_j|), the work vector scale(w_in) + |V| |s| after each sweep, |w| and w / |w| as in
xprec_step._finish.  The bound is xprec_step.bound with width = 0 and a chain of nsweeps * m roundings.

Row ownership (what the wrong variants restate):
  k_mgs_persist:    thread t of block b owns rows ((i G + b) PT + t) 2 + {0, 1}, grid-row i < NV: grid-row i = [i G PT 2, (i + 1) G PT 2)
  k_mgs_panel:      block b owns [b rpb, (b + 1) rpb), rpb = nvr DT 2, nvr = ceil(ld / (G DT 2)), DT = 512 data threads (448: lag kernel)"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

from xprec_step import LD, _finish, Step, bound, excess, skewed_basis   # noqa: F401  (re-exported for the tests)

KK_SUB = 512
PARK_BYTES = 160 * 1024 - 256     # LDS a persistent block may park rows in (persist_park)
PERSIST_NR = 9                    # KK_PERSIST_NR
PANEL_DT, LAG_DT = 512, 448       # data threads per block: k_mgs_panel, k_mgs_panel_lag
PANEL_NVMID = 8                   # KK_PANEL_NVMID


def slab_ld(n: int) -> int:
    """leading dimension of a kk_basis slab (kk_basis_create): n rounded up to 512, an odd number of 512-row chunks"""
    ld = -(-n // KK_SUB) * KK_SUB
    return ld + KK_SUB if (ld // KK_SUB) % 2 == 0 else ld


# ---- the reference ----------------------------------------------------------------------------------------------------------
@dataclass
class Sweeps:
    s: np.ndarray                     # coefficients, one row per sweep
    total: np.ndarray                 # their sum (what orthogonalize!! returns)
    w: np.ndarray                     # final work vector
    nrm: LD                           # |w|
    q: np.ndarray                     # w / |w| (w itself when |w| = 0)
    norms: List[LD] = field(default_factory=list)   # |w| after each sweep (MGSIR's pass rule)
    scale: Dict[str, object] = field(default_factory=dict)
    K: int = 0                        # the chain length handed to the bound as "m"


def mgs_sweeps(V, w, nsweeps: int, carry=None) -> Sweeps:
    """nsweeps sequential MGS sweeps of w against the columns of V, w -= s_c q_c in front when carry = (q_c, s_c)"""
    VL = np.asarray(V, dtype=LD)
    n, m = VL.shape
    aV = np.abs(np.asarray(V, dtype=np.float64))
    aG = np.tril(aV.T @ aV, -1).astype(LD)
    x = np.array(w, dtype=LD)
    xs = np.abs(x)
    if carry is not None:
        qc, sc = np.asarray(carry[0], dtype=LD), LD(carry[1])
        x = x - sc * qc
        xs = xs + abs(sc) * np.abs(qc)
    S = np.zeros((nsweeps, m), dtype=LD)
    Ss = np.zeros((nsweeps, m), dtype=LD)
    norms = []
    for k in range(nsweeps):
        for j in range(m):
            S[k, j] = np.sum(VL[:, j] * x, dtype=LD)
            x = x - S[k, j] * VL[:, j]
        Ss[k] = aV.T.astype(LD) @ xs + aG @ np.abs(S[k])
        xs = xs + aV.astype(LD) @ np.abs(S[k])
        norms.append(np.sqrt(np.sum(x * x, dtype=LD)))
    st = _finish(Step(), x, xs)
    out = Sweeps(s=S, total=S.sum(axis=0), w=x, nrm=st.beta, q=st.q, norms=norms, K=nsweeps * m)
    out.scale = {"s": Ss, "total": Ss.sum(axis=0), "w": xs, "nrm": st.scale["beta"], "q": st.scale["q"]}
    return out


def sweep_excess(dev, ref: Sweeps, key: str) -> float:
    """max |dev - ref| / bound over the elements of output `key` (bound: width 0, chain nsweeps * m)"""
    r = {"s": ref.s, "total": ref.total, "w": ref.w, "nrm": ref.nrm, "q": ref.q}[key]
    n = len(ref.w)
    return excess(dev, r, ref.scale[key], ref.K, 0, n)


# ---- the launchers' choice of shape ---------------------------------------------------------------------------------------
PERSIST_NV = {512: (8, 16, 24, 32, 40), 1024: (4, 8, 12, 16, 20)}


def persist_shape(ld: int, G: int, threads: int, lds: int, nt: int = 1, apply: bool = False):
    """(NV, NL, NR) kk_launch_mgs_persist picks (launch_persist), or None beyond the register file; `apply` only where it exists"""
    nv = -(-ld // (G * threads * 2))
    NV = next((v for v in PERSIST_NV[threads] if nv <= v), None)
    if NV is None:
        return None
    NL = min(NV, PARK_BYTES // (threads * 16))
    NR = min(NV - NL, PERSIST_NR) if threads == 512 and NV > NL else 0
    if lds == 1:
        NR = 0
    elif lds == 0:
        NL = NR = 0
    assert not apply or (threads == 512 and lds == 2 and nt and NR > 0)
    return NV, NL, NR


def panel_shape(ld: int, G: int, mgs_mode: int, panel_width: int = 0, panel_lag: int = 0):
    """(kernel, NV, P) kk_launch_mgs_panel picks: kernel 2 = k_mgs_panel, 3 = k_mgs_panel_lag; None beyond its capacity"""
    if ld > G * PANEL_DT * 2 * 16:
        return None
    strict = mgs_mode == 0
    nv = -(-ld // (G * PANEL_DT * 2))
    nvl = -(-ld // (G * LAG_DT * 2))
    if not strict and panel_lag and nvl <= 8 and (panel_width == 0 or panel_width >= 2):
        return 3, (4 if nvl <= 4 else (6 if nvl <= 6 else 8)), 2
    by_size = 3 if nv <= 4 else (2 if nv <= PANEL_NVMID else 1)
    P = 1 if strict else (min(panel_width, by_size) if panel_width > 0 else by_size)
    if nv <= 4:
        return 2, 4, min(P, 3)
    if nv <= PANEL_NVMID:
        return 2, PANEL_NVMID, min(P, 2)
    return 2, 16, 1


def instantiations():
    """every single-rank instantiation the two launchers can pick: (1, NV, NL, NR, PT, NT, APPLY), (2, NV, P), (3, NV, P)"""
    out = set()
    for PT, nvs in PERSIST_NV.items():
        for NV in nvs:
            ld = NV * PT * 2      # (G = 1, a vector that fills NV grid-rows)
            for lds in (0, 1, 2):
                for nt in (0, 1):
                    out.add((1, *persist_shape(ld, 1, PT, lds, nt), PT, nt, 0))
            if PT == 512 and NV > 24:
                out.add((1, *persist_shape(ld, 1, PT, 2, 1, True), PT, 1, 1))
    for nv in range(1, 17):
        for mode in (0, 2):
            for pw in (0, 1, 2, 3):
                for lag in (0, 1):
                    out.add(panel_shape(nv * PANEL_DT * 2, 1, mode, pw, lag))
    for nvl in range(1, 9):
        out.add(panel_shape(nvl * LAG_DT * 2, 1, 2, 0, 1))
    return sorted(out)


# ---- the GPU cases (tests/test_gpu_sweep_envelope.py; CPU pin tests/test_xprec_sweeps.py) ----------------------------------------
# a route: ("persist", threads, lds, nt) or ("panel", mgs_mode, panel_width, panel_lag)
def route_shape(route, n: int, G: int):
    """the instantiation a route runs a vector of n rows on with G blocks, in the form of instantiations()"""
    ld = slab_ld(n)
    if route[0] == "persist":
        _, threads, lds, nt = route
        return (1, *persist_shape(ld, G, threads, lds, nt), threads, nt, 0)
    _, mode, pw, lag = route
    return panel_shape(ld, G, mode, pw, lag)


def route_span(route) -> int:
    """rows of one grid-row of one block on a route: 2 x threads (k_mgs_persist), 2 x data threads (k_mgs_panel; the lag kernel, which a
    route outside the strict order with panel_lag on takes -- its `nvl` counts these grid-rows)"""
    if route[0] == "persist":
        return route[1] * 2
    return (LAG_DT if route[3] and route[1] != 0 else PANEL_DT) * 2


def bucket_top(route, nv: int) -> bool:
    """is nv the last grid-row count of the launcher bucket it falls in (the route's instantiation with the most grid-rows)?"""
    tops = PERSIST_NV[route[1]] if route[0] == "persist" else ((4, 6, 8) if route_span(route) == LAG_DT * 2 else (4, 8, 16))
    return nv in tops


def rows_for(route, nv: int, G: int, last: bool) -> int:
    """a row count whose slab makes the route's launcher see `nv` grid-rows at G blocks: the first slab that does (last grid-row holding
    512 rows, so that most blocks own nothing in it) or the last one (the grid-row all but full); n is never a multiple of 512"""
    span = G * route_span(route)
    lo, hi = (nv - 1) * span, nv * span          # ld in (lo, hi]
    for ld in (range(hi - hi % KK_SUB, lo, -KK_SUB) if last else range(lo - lo % KK_SUB + KK_SUB, hi + 1, KK_SUB)):
        if ld > lo and (ld // KK_SUB) % 2 == 1:
            assert slab_ld(ld - 37) == ld
            return ld - 37
    raise ValueError((route, nv, G))


def _persist_routes():
    for threads in (512, 1024):
        for lds in (0, 1, 2):
            for nt in (1, 0):
                yield ("persist", threads, lds, nt)


# (a) every instantiation: G rotating through 1, 2, 3, the vector filling most of its NV grid-rows; m = 6
def cases_a():
    out = []
    seen = set()
    k = 0
    for route in list(_persist_routes()):
        for NV in PERSIST_NV[route[1]]:
            G = (1, 2, 3)[k % 3]
            n = rows_for(route, NV, G, last=(k % 2 == 0))
            shape = route_shape(route, n, G)
            if shape in seen:
                continue
            seen.add(shape)
            out.append((route, G, n, 6))
            k += 1
    for route, nvs in ((("panel", 0, 0, 0), (4, 8, 16)), (("panel", 2, 1, 0), (4, 8)), (("panel", 2, 2, 0), (4, 8)), (("panel", 2, 0, 0), (4,)),
                       (("panel", 2, 0, 1), (4, 6, 8))):
        for nv in nvs:
            G = (1, 2, 3)[k % 3]
            n = rows_for(route, nv, G, last=(k % 2 == 0))
            shape = route_shape(route, n, G)
            if shape not in seen:
                seen.add(shape)
                out.append((route, G, n, 7))
            k += 1
    return out


# (b) row-count edges: the first and the last nv each instantiation takes, on the default route of each kernel, G in 1, 2, 3, 7, 64, 65 and
# the whole chip (None) -- at most ~2.7 M rows, small m
EDGE_FAMILIES = [
    (("persist", 512, 2, 1), [(1, None), (8, None), (9, None), (16, 65), (17, 64), (24, 7), (25, 3), (32, 2), (33, 1), (40, 65)]),
    (("persist", 1024, 2, 1), [(1, None), (4, None), (5, 65), (8, 64), (9, 7), (12, 3), (13, 2), (16, 1), (17, 65), (20, 64)]),
    (("panel", 2, 0, 0), [(1, None), (4, None), (5, 7), (8, None), (9, 65), (16, 64)]),
    (("panel", 2, 0, 1), [(1, None), (4, 3), (5, 65), (6, 2), (7, 7), (8, None)]),
]


def edge_case(route, nv: int, G: int):
    """(n, m) of a row-count edge: nv at the top of its bucket takes the last slab, anything else the first; m = 3 above 400 k rows"""
    n = rows_for(route, nv, G, last=bucket_top(route, nv))
    return n, (3 if n > 400_000 else 5)


def edges():
    """(route, G, nv) of every row-count edge; G = None: the whole chip (resolved where the device is known)"""
    return [(route, G, nv) for route, es in EDGE_FAMILIES for nv, G in es]


def cases_b(all_cus: int):
    """the row-count edges as (route, G, n, m) on a chip of `all_cus` CUs"""
    out = []
    for route, G, nv in edges():
        G = all_cus if G is None else G
        out.append((route, G, *edge_case(route, nv, G)))
    return out


# (c) basis sizes on the default instantiations, two NV per kernel (panel: P = 3 and P = 2), G = 1
CASES_C_M = [1, 2, 3, 64, 65, 128, 129, 255, 256]
CASES_C_SHAPES = [(("persist", 512, 2, 1), 8), (("persist", 512, 2, 1), 24), (("panel", 2, 0, 0), 4), (("panel", 2, 0, 0), 8)]


def cases_c():
    return [(route, 1, rows_for(route, nv, 1, last=True), m) for route, nv in CASES_C_SHAPES for m in CASES_C_M]


def spread_for(m: int) -> float:
    """overlaps of the skewed basis: 0.03 (xprec_step), smaller for wide bases so that ||E|| stays ~0.5 and kappa(V) small"""
    return min(0.03, 0.25 / math.sqrt(m))


def sweep_inputs(n: int, m: int):
    """(V, w) of a case: V skewed (unit columns, overlaps ~1e-2), w = 8 V c + a unit-size out-of-span part -- the MGS coefficients are
    O(10) and differ from the CGS ones by the overlaps times that: what a stale row, a missing correction or a dropped axpy moves"""
    seed = 7919 * m + n
    V = skewed_basis(n, m, seed, spread_for(m))
    rng = np.random.default_rng(seed + 1)
    c = 8.0 * (1.0 + rng.random(m)) * rng.choice([-1.0, 1.0], m)
    w = V @ c + rng.standard_normal(n) / math.sqrt(n) * 4.0
    return V, w


def mgsir_eta(ref2: Sweeps, w) -> float:
    """an eta for which MGSIR takes exactly two passes: |w1| < eta |w0| and |w2| > eta |w1|, each by 20 % at least (the rounding of the
    norms is ~1e-15 of them: the pass count is unambiguous)"""
    n0 = float(np.linalg.norm(w))
    r1, r2 = float(ref2.norms[0]) / n0, float(ref2.norms[1] / ref2.norms[0])
    eta = math.sqrt(r1 * r2)
    assert r1 < 0.8 * eta and r2 > 1.25 * eta, (r1, r2)
    return eta


# ---- wrong variants (f64: their errors are orders of magnitude above the rounding they would carry) --------------------------------
def owned_rows(route, n: int, G: int, b: int) -> np.ndarray:
    """rows block b owns"""
    ld = slab_ld(n)
    if route[0] == "persist":
        PT = route[1]
        span = G * PT * 2
        nv = -(-ld // span)
        rows = np.concatenate([np.arange((i * G + b) * PT * 2, (i * G + b + 1) * PT * 2) for i in range(nv)])
    else:
        DT = LAG_DT if route_shape(route, n, G)[0] == 3 else PANEL_DT
        nvr = -(-ld // (G * DT * 2))
        rows = np.arange(b * nvr * DT * 2, (b + 1) * nvr * DT * 2)
    return rows[rows < n]


def last_grid_row(route, n: int, G: int) -> np.ndarray:
    """rows of the last (partial) grid-row: persist the last G PT 2 span, panel the last row of DT double2 of the last block owning rows"""
    ld = slab_ld(n)
    if route[0] == "persist":
        span = G * route[1] * 2
        lo = (-(-n // span) - 1) * span
    else:
        DT = LAG_DT if route_shape(route, n, G)[0] == 3 else PANEL_DT
        rpb = -(-ld // (G * DT * 2)) * DT * 2
        b = (n - 1) // rpb
        lo = b * rpb + ((n - 1 - b * rpb) // (DT * 2)) * DT * 2
    return np.arange(lo, n)


def sweeps_variant(V, w, nsweeps: int, variant: str, route, G: int, carry=None, P: int = 1):
    """the wrong forms, in f64:
      stale_parked        grid-rows < NL + NR (persist) take q_{j-1} in the axpy of step j (the park not refreshed)
      tail_dropped        the rows of the last grid-row are never updated
      block_missing       one block's partial missing from one reduction (the last vector of the first sweep, the last block owning rows)
      panel_cgs           no in-panel correction: every coefficient of a panel of P >= 2 from w as it was before the panel
      carry_dropped       the pending w -= s_c q_c left out
      restart_from_input  the second sweep starts from the input w0 instead of the first sweep's result
    returns (coefficients per sweep, w)"""
    V = np.asarray(V, dtype=np.float64)
    n, m = V.shape
    x = np.array(w, dtype=np.float64)
    if carry is not None and variant != "carry_dropped":
        x = x - carry[1] * np.asarray(carry[0])
    w0 = x.copy()
    keep = np.zeros(n, dtype=bool)
    parked = np.zeros(n, dtype=bool)
    if variant == "tail_dropped":
        keep[last_grid_row(route, n, G)] = True
    if variant == "stale_parked":
        shape = route_shape(route, n, G)
        span = G * route[1] * 2
        parked[: min(n, (shape[2] + shape[3]) * span)] = True
    miss = None
    if variant == "block_missing":
        bl = max(b for b in range(G) if len(owned_rows(route, n, G, b)))
        miss = owned_rows(route, n, G, bl)
    S = np.zeros((nsweeps, m))
    prev = None
    for k in range(nsweeps):
        if variant == "restart_from_input" and k == 1:
            x = w0.copy()
        j = 0
        while j < m:
            p = P if variant == "panel_cgs" else 1
            xb = x.copy()
            for jj in range(j, min(m, j + p)):
                src = xb if variant == "panel_cgs" else x
                s = float(V[:, jj] @ src)
                if miss is not None and k == 0 and jj == m - 1:
                    s -= float(V[miss, jj] @ src[miss])
                S[k, jj] = s
                q = V[:, jj]
                if variant == "stale_parked" and prev is not None:
                    q = np.where(parked, V[:, prev], q)
                upd = x - s * q
                x = np.where(keep, x, upd)
                prev = jj
            j += p
    return S, x


# (d) one expand! per route: Lanczos MGS2 (the pending w -= alpha0 v rides into the sweep as the kernel's carry) and Arnoldi MGS, MGS2 on a
# shifted Laplacian, G = 1; then the in-kernel apply (k_mgs_persist<.., APPLY>): value-free Laplacian with an even line length, NV 32 and 40
# at 512 threads, and an odd line length for contrast (no apply)
CASES_D_ROUTES = [("persist", 512, 2, 1), ("persist", 1024, 2, 1), ("persist", 512, 0, 0), ("panel", 0, 0, 0), ("panel", 2, 0, 0), ("panel", 2, 0, 1)]
CASES_D_GRID, CASES_D_M = (96, 100), 7
CASES_D_APPLY = [((128, 208), True), ((128, 300), True), ((127, 300), False)]


def lanczos_carry(A, V, beta_old):
    """the work vector and the pending axpy the strict Lanczos MGS2 step hands its sweep: w0 = A v - beta v_prev, carry (v, alpha0 = <v, w0>)
    (lanczos.jl:326-328), in f64 as the device forms them (inputs of the CPU pin's carry_dropped variant)"""
    m = V.shape[1]
    v, vprev = V[:, m - 1], V[:, m - 2]
    w0 = A @ v - beta_old * vprev
    return w0, (v, float(v @ w0))
