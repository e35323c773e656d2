"""GPU: every path of the symmetric eigensolver (tf_eigh.hip.h: eigh, eigh_blocked; tf_jacobi.hip.h) against LAPACK (numpy.linalg.eigh),
reached through tf_diagonalise with X = I (eps, C = eigh(A)) -- np.linalg.eigh in diagonalise_Fock_matrix (scf:244).

Paths: the in-LDS Jacobi on the full matrix (2 <= n <= 64), rocsolver_dsyevd (n = 1, n > 64), the batched in-LDS Jacobi over the x/y parity
blocks of a z-axis diatomic (n >= 40, blocks <= 64) and rocsolver_dsyevd_strided_batched over the blocks padded to the largest one (a block
above 64).  A context offers the blocks only when its tensor is built; the class sizes come from the basis: per atom class 0 = s + p + 2d + 2f,
classes 1 and 2 = p + d + 2f each, class 3 = d + f.

Bars (Weyl and the backward error of a stable solver, c n eps |A| with c = 10, where 2 was the most measured on any path): eigenvalues and
residual |A V - V L| within 10 n eps |A|, |V^T V - I| within 10 n eps; on the blocked paths exact zeros outside a vector's class, and exact ties
between blocks in block order; for every cluster of (near-)degenerate eigenvalues the spectral projector within 10 n eps |A| / gap of
LAPACK's (the vectors inside a cluster are arbitrary)."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tuna_amd import molecule as mol
from tuna_amd._lib import TunaError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))


# ---- matrices -------------------------------------------------------------------------------------------------------------------
def _orth(rng, m):
    q, r = np.linalg.qr(rng.standard_normal((m, m)))
    return q * np.sign(np.diag(r))


def _from_spectrum(rng, lam):
    q = _orth(rng, len(lam))
    a = (q * lam) @ q.T
    return 0.5 * (a + a.T)


def spectrum_matrix(kind, m, rng):
    """A symmetric m x m matrix of the named spectral type."""
    if m == 0:
        return np.zeros((0, 0))
    if kind == "gauss":
        g = rng.standard_normal((m, m))
        return 0.5 * (g + g.T)
    if kind == "multiplet":                                   # exact (in exact arithmetic) triples
        return _from_spectrum(rng, np.repeat(rng.standard_normal((m + 2) // 3), 3)[:m])
    if kind == "near_degenerate":                             # pairs 1e-10 apart
        b = np.repeat(rng.standard_normal((m + 1) // 2), 2)[:m]
        return _from_spectrum(rng, b + 1e-10 * (np.arange(m) % 2))
    if kind == "graded":                                      # |lambda| from 1e-12 to 1e4, both signs
        return _from_spectrum(rng, np.logspace(-12, 4, m) * rng.choice([-1.0, 1.0], m))
    if kind == "diagonal":                                    # apq == 0 from the start
        return np.diag(rng.standard_normal(m))
    if kind == "tau_zero":                                    # equal diagonal, tiny off-diagonal: tau = 0 in every first rotation
        e = 1e-9 * rng.standard_normal((m, m))
        e = 0.5 * (e + e.T)
        np.fill_diagonal(e, 0.0)
        return 1.5 * np.eye(m) + e
    if kind == "zero":
        return np.zeros((m, m))
    if kind == "rank_one":
        v = rng.standard_normal(m)
        return np.outer(v, v)
    if kind == "gershgorin":                                  # every eigenvalue on the Gershgorin bound (the padding sits 1 % above it)
        return 3.0 * np.eye(m)
    if kind == "diag_dominant":                               # max |a| close to the largest row sum (the Gershgorin bound)
        g = 1e-3 * rng.standard_normal((m, m))
        return np.diag(rng.uniform(-1.0, 1.0, m)) + 0.5 * (g + g.T)
    if kind == "negative_definite":
        return -_from_spectrum(rng, rng.uniform(1.0, 10.0, m))
    raise ValueError(kind)


SPECTRA = ("gauss", "multiplet", "near_degenerate", "graded", "diagonal", "tau_zero", "zero", "rank_one", "gershgorin",
           "negative_definite", "diag_dominant")


# ---- checks ---------------------------------------------------------------------------------------------------------------------
WORST = {}            # path -> largest ratios seen (printed at the end of the module with -s)


def _note(path, **ratios):
    w = WORST.setdefault(path, {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), float(v))


def check_eigh(A, eps, V, path, label, cls=None, c=10):
    """eps, V (columns) from the device against LAPACK on the full matrix A; bars c n eps |A|."""
    n = A.shape[0]
    ref, Vr = np.linalg.eigh(A)
    normA = float(np.abs(ref).max()) if n else 0.0
    eps_m = np.finfo(float).eps
    tol = c * n * eps_m * normA                               # (measured on MI355X: at most 1.4 n eps |A| on any path)
    assert np.all(np.isfinite(eps)) and np.all(np.isfinite(V)), label
    assert np.all(np.diff(eps) >= 0), (label, "eigenvalues not ascending")
    de = float(np.abs(eps - ref).max())
    res = float(np.abs(A @ V - V * eps).max())
    orth = float(np.abs(V.T @ V - np.eye(n)).max())
    assert de <= tol, (label, "eigenvalue error", de, tol)
    assert res <= tol, (label, "residual", res, tol)
    assert orth <= c * n * eps_m, (label, "orthogonality", orth)   # (measured: at most 2.0 n eps)
    scale = max(n * eps_m * normA, 1e-300)
    _note(path, eig_err=de / scale, residual=res / scale, orth=orth / (n * eps_m))
    # clusters of (near-)degenerate eigenvalues: the projector onto each
    if n > 1 and normA > 0:
        cut = 1e-8 * normA
        starts = [0] + [k for k in range(1, n) if ref[k] - ref[k - 1] > cut] + [n]
        for a, b in zip(starts[:-1], starts[1:]):
            if b - a == n:
                continue
            gap = min(ref[a] - ref[a - 1] if a > 0 else np.inf, ref[b] - ref[b - 1] if b < n else np.inf)
            P = V[:, a:b] @ V[:, a:b].T
            Pr = Vr[:, a:b] @ Vr[:, a:b].T
            dp = float(np.abs(P - Pr).max())
            assert dp <= c * n * eps_m * normA / gap, (label, "projector of cluster", (a, b), dp, gap)   # (measured: 0.7)
            _note(path, projector=dp * gap / scale)
    if cls is not None:
        # blocked solve: every vector lives in one class (exact zeros elsewhere); exact ties between blocks keep the block order
        vc = np.full(n, -1)
        for k in range(n):
            nz = np.flatnonzero(V[:, k])
            assert nz.size == 0 or np.all(cls[nz] == cls[nz[0]]), (label, "vector leaves its class", k)
            vc[k] = cls[nz[0]] if nz.size else -1
        for k in range(n - 1):
            if eps[k] == eps[k + 1]:
                assert vc[k] <= vc[k + 1], (label, "tie order between blocks", k, vc[k], vc[k + 1])


# ---- contexts -------------------------------------------------------------------------------------------------------------------
def ao_classes(eng):
    """x/y parity class of every spherical AO of the context, in its order ((lx & 1) | (ly & 1) << 1 of its Cartesian components)."""
    U = eng.sph_matrix()
    lmn = np.asarray(eng.aos.lmn)
    c_cart = (lmn[:, 0] & 1) | ((lmn[:, 1] & 1) << 1)
    cls = np.empty(U.shape[0], dtype=np.int64)
    for i in range(U.shape[0]):
        cs = set(c_cart[np.flatnonzero(np.abs(U[i]) > 1e-12)].tolist())
        assert len(cs) == 1
        cls[i] = cs.pop()
    return cls


def expected_sizes(counts):
    s = np.zeros(4, dtype=int)
    for ns, npp, nd, nf in counts:
        s += [ns + npp + 2 * nd + 2 * nf, npp + nd + 2 * nf, npp + nd + 2 * nf, nd + nf]
    return s


# name -> ((s, p, d, f) of atom A, of atom B), path the default solver takes
CONFIGS = {
    "n39_below_nmin": (((5, 3, 1, 0), (6, 3, 1, 0)), "jacobi"),           # 21 / 8 / 8 / 2: n = 39 < TF_EIGH_BLOCKS_NMIN
    "n40_blocked": (((5, 3, 1, 0), (7, 3, 1, 0)), "blocked_jacobi"),      # 22 / 8 / 8 / 2: n = 40
    "mmax64": (((20, 12, 0, 0), (20, 12, 0, 0)), "blocked_jacobi"),      # 64 / 24 / 24: n = 112
    "mmax65": (((20, 12, 0, 0), (21, 12, 0, 0)), "blocked_dsyevd"),      # 65 / 24 / 24: n = 113
    "block_of_one": (((12, 5, 1, 0), (12, 5, 0, 0)), "blocked_jacobi"),  # 36 / 11 / 11 / 1: n = 59
    "one_class_dominates": (((30, 1, 0, 0), (30, 1, 0, 0)), "dsyevd"),   # 62 / 2 / 2: 4 mmax > 3 n, n = 66
}

_ENGINES = {}


@pytest.fixture(scope="module")
def engines():
    from tuna_amd.engine import Engine
    yield _ENGINES
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    print("\n[test_gpu_eigh] worst deviations in units of n eps |A| (orthogonality: n eps):")
    for path, w in sorted(WORST.items()):
        print(f"  {path}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(w.items())))


def plain_engine(engines):
    from tuna_amd.engine import Engine
    if "plain" not in engines:
        engines["plain"] = Engine(0)
    return engines["plain"]


def sym_engine(engines, name):
    from tuna_amd.engine import Engine
    if name not in engines:
        (ca, cb), _ = CONFIGS[name]
        atoms = mol.make_atoms(["N", "O"], 2.2)
        shells = mol.build_shells(atoms, {7: mol.even_tempered_basis(*ca), 8: mol.even_tempered_basis(*cb)})
        eng = Engine(0)
        eng.set_basis(mol.expand_cartesian_aos(shells)).build_eri(True)
        eng.cls = ao_classes(eng)
        assert list(np.bincount(eng.cls, minlength=4)) == list(expected_sizes((ca, cb))), name
        engines[name] = eng
    return engines[name]


def class_diagonal(cls, kind, rng, same_pi=True):
    """Random symmetric matrix, exactly zero between different classes; classes 1 and 2 (px / py) get the same block when same_pi."""
    n = len(cls)
    A = np.zeros((n, n))
    blocks = {}
    for c in range(4):
        idx = np.flatnonzero(cls == c)
        if c == 2 and same_pi and len(idx) == len(np.flatnonzero(cls == 1)):
            B = blocks[1]
        else:
            B = spectrum_matrix(kind, len(idx), rng)
        blocks[c] = B
        A[np.ix_(idx, idx)] = B
    return A


def solve(eng, A):
    return eng.diagonalise(A, np.eye(A.shape[0]))


# ---- the full-matrix paths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 63, 64, 65, 100])
def test_full_matrix_paths_against_lapack(engines, n):
    """No symmetry offered (a context without a tensor): the in-LDS Jacobi for 2 <= n <= 64 (odd n: the bye of the tournament
    ordering), rocsolver_dsyevd for n = 1 and n > 64."""
    eng = plain_engine(engines)
    path = "jacobi" if 2 <= n <= 64 else "dsyevd"
    rng = np.random.default_rng(1000 + n)
    s0 = eng.eigh_stats()
    for kind in SPECTRA:
        A = spectrum_matrix(kind, n, rng)
        eps, V = solve(eng, A)
        check_eigh(A, eps, V, path, f"n={n} {kind}")
    s1 = eng.eigh_stats()
    assert s1 == s0                                           # no blocked solve, no fallback


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_parity_block_paths_against_lapack(engines, name):
    """Class-diagonal matrices in bases whose class sizes sit at the route boundaries: n = 39 / 40 around TF_EIGH_BLOCKS_NMIN, largest
    block 64 (batched Jacobi) / 65 (padded dsyevd_strided_batched), a block of one function, and one class holding more than 3/4 of the
    basis (declined: nothing to gain).  The px / py blocks are equal, as in every pi shell: exact ties across blocks."""
    eng = sym_engine(engines, name)
    cls = eng.cls
    path = CONFIGS[name][1]
    blocked = path.startswith("blocked")
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    for kind in SPECTRA + ("gauss_distinct_pi",):
        A = class_diagonal(cls, "gauss" if kind == "gauss_distinct_pi" else kind, rng, same_pi=kind != "gauss_distinct_pi")
        s0 = eng.eigh_stats()
        eps, V = solve(eng, A)
        s1 = eng.eigh_stats()
        assert s1["blocked_solves"] == s0["blocked_solves"] + (1 if blocked else 0), (name, kind, s0, s1)
        assert s1["blocked_declined"] == s0["blocked_declined"] and s1["jacobi_fallbacks"] == s0["jacobi_fallbacks"], (name, kind)
        # the padded batch: a padding just above the spectrum (1.01 x the Gershgorin bound) leaves it as accurate as dsyevd on each block
        # (measured at most 0.11 n eps |A|); one far above it (n max|a|) costs up to a factor n in absolute accuracy
        check_eigh(A, eps, V, path, f"{name} {kind}", cls=cls if blocked else None, c=1 if path == "blocked_dsyevd" else 10)


@pytest.mark.parametrize("name", ["n40_blocked", "mmax65"])
def test_cross_class_threshold(engines, name):
    """eigh_blocked accepts a matrix whose largest element between classes is at most 1e-14 of its largest element (and then solves the
    blocks alone: the result must still match LAPACK on the full matrix), and declines above -- the full matrix is solved."""
    eng = sym_engine(engines, name)
    cls = eng.cls
    rng = np.random.default_rng(7)
    A = class_diagonal(cls, "gauss", rng, same_pi=False)
    i, j = int(np.flatnonzero(cls == 0)[1]), int(np.flatnonzero(cls == 1)[0])
    amax = np.abs(A).max()
    for rel, accepted in ((0.5e-14, True), (2e-14, False)):
        B = A.copy()
        B[i, j] = B[j, i] = rel * amax
        s0 = eng.eigh_stats()
        eps, V = solve(eng, B)
        s1 = eng.eigh_stats()
        if accepted:
            assert s1["blocked_solves"] == s0["blocked_solves"] + 1 and s1["blocked_declined"] == s0["blocked_declined"]
            check_eigh(B, eps, V, "blocked_cross_accepted", f"{name} cross {rel}")
        else:
            assert s1["blocked_solves"] == s0["blocked_solves"] and s1["blocked_declined"] == s0["blocked_declined"] + 1
            check_eigh(B, eps, V, "blocked_cross_declined", f"{name} cross {rel}")


@pytest.mark.parametrize("scale", [1e100, 1e-100, 1e200, 1e-200])
def test_extreme_scales(engines, scale):
    """The same matrices at 1e+-100 and 1e+-200 on every path.  The Jacobi stopping test squares the elements; beyond ~1e+-154 that
    overflows or underflows, and without a power-of-two scaling the kernel would return the diagonal with no rotation at all; rocSOLVER's
    dsyevd does not scale either (unscaled: eigenvalues wrong by 100 % at 1e-100 and 1e-200, no convergence at 1e200)."""
    rng = np.random.default_rng(11)
    cases = [(plain_engine(engines), 32, None, "jacobi"), (plain_engine(engines), 100, None, "dsyevd")]
    for name in ("n40_blocked", "mmax65"):
        e = sym_engine(engines, name)
        cases.append((e, None, e.cls, CONFIGS[name][1]))
    for eng, n, cls, path in cases:
        A = spectrum_matrix("gauss", n, rng) if cls is None else class_diagonal(cls, "gauss", rng)
        eps, V = solve(eng, scale * A)
        eps1, V1 = solve(eng, A)
        check_eigh(scale * A, eps, V, path + "_scaled", f"{path} x {scale:g}", cls=cls)
        assert np.abs(eps / scale - eps1).max() <= 10 * len(eps) * np.finfo(float).eps * np.abs(eps1).max()


@pytest.mark.parametrize("where", ["jacobi", "dsyevd", "blocked"])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_is_an_error(engines, where, bad):
    """np.linalg.eigh raises LinAlgError on a matrix with a NaN or an infinity (caught at scf:244); so does every path here (TF_ELINALG),
    instead of returning vectors with TF_OK."""
    if where == "blocked":
        eng = sym_engine(engines, "n40_blocked")
        A = class_diagonal(eng.cls, "gauss", np.random.default_rng(3))
    else:
        eng = plain_engine(engines)
        A = spectrum_matrix("gauss", 16 if where == "jacobi" else 80, np.random.default_rng(3))
    A[1, 1] = bad
    with pytest.raises(TunaError) as ei:
        solve(eng, A)
    assert ei.value.code == -5, ei.value                          # TF_ELINALG
    with pytest.raises(TunaError):
        eng.orthogonaliser(A)
    eps, V = solve(eng, np.eye(A.shape[0]))                       # the context is still usable
    assert np.abs(eps - 1.0).max() == 0.0


def test_orthogonaliser_paths(engines):
    """tf_orthogonaliser (kernel:756-816) on full and blocked paths against the LAPACK restatement: X = S^-1/2, S^-1, smallest eigenvalue."""
    from oracle import scf_oracle as so
    rng = np.random.default_rng(5)
    for eng, cls in ((plain_engine(engines), None), (sym_engine(engines, "mmax64"), "blk"), (sym_engine(engines, "mmax65"), "blk")):
        n = 50 if cls is None else eng.N
        if cls is None:
            q = _orth(rng, n)
            S = (q * np.logspace(-5, 0.5, n)) @ q.T
        else:
            A = class_diagonal(eng.cls, "gauss", rng)
            S = A @ A.T / n + 1e-4 * np.eye(n)
        S = 0.5 * (S + S.T)
        X, sm, Si = eng.orthogonaliser(S)
        Xo, smo, Sio = so.orthogonaliser(S)
        kappa = np.linalg.cond(S)
        assert abs(sm - smo) <= 1e-13 * n * np.abs(np.linalg.eigvalsh(S)).max()
        assert np.abs(X - Xo).max() <= 1e-13 * n * kappa * np.abs(Xo).max()
        assert np.abs(Si - Sio).max() <= 1e-13 * n * kappa * np.abs(Sio).max()
        assert np.abs(X @ S @ X - np.eye(n)).max() <= 1e-13 * n * kappa


# ---- solver failures --------------------------------------------------------------------------------------------------------------
_CAP_CODE = r'''
import sys, json, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(here)r)
import test_gpu_eigh as t
from tuna_amd.engine import Engine
from tuna_amd._lib import TunaError
out = {}
engines = {}
eng = t.plain_engine(engines)
rng = np.random.default_rng(21)
A = t.spectrum_matrix("gauss", 32, rng)
s0 = eng.eigh_stats(); eps, V = t.solve(eng, A); s1 = eng.eigh_stats()
t.check_eigh(A, eps, V, "jacobi_capped", "n=32 with the sweep cap at 1")
out["full"] = [s0, s1]
e2 = t.sym_engine(engines, "mmax64")
B = t.class_diagonal(e2.cls, "gauss", rng)
s0 = e2.eigh_stats(); eps, V = t.solve(e2, B); s1 = e2.eigh_stats()
t.check_eigh(B, eps, V, "blocked_capped", "mmax64 with the sweep cap at 1")
out["blocked"] = [s0, s1]
# a native cycle whose exact solves are the Jacobi kernel: a solve that did not converge is an error, not a result
from conftest import atom_arrays, make_system
from oracle import scf_oracle as so
from tuna_amd import molecule as mol
atoms, shells, aos, nocc = make_system("n2_sto3g")
e3 = Engine(0)
e3.set_basis(aos).build_eri(True)
xyz, chg, org = atom_arrays(atoms)
S, T, V_, _, _ = e3.one_electron(xyz, chg, org, spherical=True)
X, _, _ = so.orthogonaliser(S)
P0, E0 = so.core_guess(T, V_, X, nocc)
try:
    r = e3.scf_rhf(S, T, V_, P0, E0, nocc, mol.nuclear_repulsion(atoms), X=X, conv="tight", damping="none", n_atom_ao=[5, 5])
    out["cycle"] = ["ok", r["energy"]]
except TunaError as e:
    out["cycle"] = [str(e), e.code]
for e in list(engines.values()) + [e3]:
    e.close()
print(json.dumps(out))
'''


def test_jacobi_that_does_not_converge_is_not_a_result():
    """With the sweep cap of the Jacobi kernels at 1 (TF_JACOBI_SWEEPS, read once per process: a child process) ordinary matrices do not
    converge.  Their `info` must be read: the full-matrix solve is repeated by dsyevd, a blocked solve declines to the full matrix
    (both give LAPACK's eigenpairs, and the counters show the route), and a native cycle stops with TF_ELINALG."""
    env = dict(os.environ)
    env["TF_JACOBI_SWEEPS"] = "1"
    code = _CAP_CODE % {"root": ROOT, "here": HERE}
    o = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert o.returncode == 0, o.stderr[-3000:]
    out = json.loads(o.stdout.strip().splitlines()[-1])
    s0, s1 = out["full"]
    assert s1["jacobi_fallbacks"] == s0["jacobi_fallbacks"] + 1
    s0, s1 = out["blocked"]
    assert s1["blocked_declined"] == s0["blocked_declined"] + 1 and s1["blocked_solves"] == s0["blocked_solves"]
    msg, code_ = out["cycle"]
    assert code_ == -5 and "did not converge" in msg, out["cycle"]


# ---- one context across sizes and spins -----------------------------------------------------------------------------------------
def test_one_context_across_sizes_and_spins():
    """What the eigensolver keeps between calls (tables of the parity blocks, grow-only blocks, the refinement start of each spin) must
    not leak from one problem into the next: one context runs RHF on N2/cc-pVTZ (n = 60: blocked Jacobi, in-LDS refinement), RHF on
    Ar2/cc-pVQZ (n = 118: blocks <= 64, blocked refinement), UHF on the O2 triplet in cc-pVDZ (both spin slots), RHF on N2/STO-3G
    (n = 10: tables and blocks shrink) and N2/cc-pVTZ again, with set_basis and build_eri between them; every run equals the same run on
    a fresh context: iteration count, `converged`, the eigensolver's path counters, and the energy within the bar
    tests/test_host_logic.py has for the lockstep batch (1e-10)."""
    from conftest import atom_arrays, make_system, make_uhf_system
    from tuna_amd.engine import Engine

    def run(eng, tag):
        if tag.startswith("o2_"):
            atoms, shells, aos, na, nb = make_uhf_system(tag)
        else:
            atoms, shells, aos, na = make_system(tag)
            nb = None
        eng.set_basis(aos).build_eri(True)
        xyz, chg, org = atom_arrays(atoms)
        S, T, V, _, _ = eng.one_electron(xyz, chg, org, spherical=True)
        X, _, _ = eng.orthogonaliser(S)
        _, C0 = eng.diagonalise(T + V, X)
        nao = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
        vnn = mol.nuclear_repulsion(atoms)
        conv = "extreme" if eng.N <= 64 else "tight"
        s0 = eng.eigh_stats()
        if nb is None:
            P0 = 2.0 * C0[:, :na] @ C0[:, :na].T
            P0 = 0.5 * (P0 + P0.T)
            r = eng.scf_rhf(S, T, V, P0, float(np.sum(P0 * (T + V))), na, vnn, X=X, conv=conv, damping="dynamic", n_atom_ao=nao)
        else:
            Pa, Pb = C0[:, :na] @ C0[:, :na].T, C0[:, :nb] @ C0[:, :nb].T
            r = eng.scf_uhf(S, T, V, 0.5 * (Pa + Pa.T), 0.5 * (Pb + Pb.T), float(np.sum((Pa + Pb) * (T + V))), na, nb, vnn, X=X, conv=conv,
                            damping="dynamic", n_atom_ao=nao)
        s1 = eng.eigh_stats()
        return eng.N, r, {k: s1[k] - s0[k] for k in s0}

    # tag, n, blocked solves expected
    order = (("c2_n2_ccpvtz", 60, True), ("c3_ar2_ccpvqz", 118, True), ("o2_triplet_ccpvdz", 28, False), ("n2_sto3g", 10, False),
             ("c2_n2_ccpvtz", 60, True))
    fresh = {}
    for tag, _, _ in order:
        if tag not in fresh:                                      # the reference runs: computed once, left unchanged
            with Engine(0) as e:
                fresh[tag] = run(e, tag)
    with Engine(0) as eng:
        for tag, n, blocked in order:
            N, r, paths = run(eng, tag)
            N0, r0, paths0 = fresh[tag]
            dE = abs(r["energy"] - r0["energy"])
            print(f"{tag}: n {N}, {r['n_iter']} iterations, |dE| {dE:.3e} ({'equal to the last bit' if r['energy'] == r0['energy'] else 'NOT bit-equal'}), {paths}")
            assert N == N0 == n
            assert r["converged"] and r0["converged"] and r["n_iter"] == r0["n_iter"], (tag, r["n_iter"], r0["n_iter"])
            assert dE < 1e-10, (tag, r["energy"], r0["energy"])
            assert paths == paths0, (tag, paths, paths0)
            assert paths["refined_solves"] > 0, (tag, paths)
            assert (paths["blocked_solves"] > 0) == blocked, (tag, paths)
