"""CPU: the NumPy MP2 density of tests/mp2_density_reference.py against the reference program's own densities
(tests/golden/mp2_density_systems.npz, tools/make_golden_mp2_density.py): every element of the unrelaxed and the relaxed P in the MO and
the AO basis and of z within 1e-12, for MP2 and SCS-MP2 on all six systems; the trace, the symmetry, the natural occupations and the
dipole moment; and the conditioning the golden tool promises (cond(A + B) 1e-15 max|z| < 1e-11).  Then the cases of
tests/test_gpu_mp2_density_shapes.py (random orbitals, no golden): the restatement from MO blocks against the dense one, the checker
against its own longdouble evaluation at a tenth of the device bound, and the conditioning of every case (D < 0, lambda_min(A + B) > 1,
cond(A + B) < 50: measured lambda_min 1.32 ... 1.51 and cond 19.0 ... 27.1 at N = 60, 10.9 ... 11.0 and 1.8 ... 2.0 at N = 10)."""
import numpy as np
import pytest

import mp2_density_reference as mr
from conftest import R_H2, R_N2
from tuna_amd import molecule as mol

SYSTEMS = {"h2_sto3g": (["H", "H"], R_H2, "STO-3G"), "co_sto3g": (["C", "O"], mol.angstrom_to_bohr(1.128), "STO-3G"),
           "co_631g": (["C", "O"], mol.angstrom_to_bohr(1.128), "6-31G"), "n2_ccpvdz": (["N", "N"], R_N2, "cc-pVDZ"),
           "n2_ccpvtz": (["N", "N"], R_N2, "cc-pVTZ"), "f2_631g": (["F", "F"], mol.angstrom_to_bohr(1.412), "6-31G")}
METHODS = ("mp2", "scs")
TOL = 1e-12


def split(z):
    out = {}
    for key in z.files:
        tag, name = key.split("__", 1)
        out.setdefault(tag, {})[name] = z[key]
    return out


def system(tag):
    sym, R, basis = SYSTEMS[tag]
    atoms = mol.make_atoms(sym, R)
    shells = mol.build_shells(atoms, basis)
    return atoms, shells, mol.expand_cartesian_aos(shells)


@pytest.fixture(scope="module")
def dens_golden(golden):
    return split(golden("mp2_density_systems"))


def test_golden_file_holds_the_systems(dens_golden):
    assert set(dens_golden) == set(SYSTEMS)
    shapes = {tag: (int(g["n_occ"]), len(g["eps"]) - int(g["n_occ"])) for tag, g in dens_golden.items()}
    assert shapes["h2_sto3g"] == (1, 1) and shapes["co_sto3g"][1] < shapes["co_sto3g"][0]
    assert shapes["f2_631g"][0] ** 2 > 64 and sum(shapes["f2_631g"]) <= 30 and sum(shapes["n2_ccpvtz"]) == 60
    for tag, g in dens_golden.items():
        for m in METHODS:
            assert float(g[f"{m}_cond"]) * 1e-15 * np.abs(g[f"{m}_z"]).max() < 1e-11, (tag, m)
    assert float(dens_golden["co_631g"]["scs_c_os"]) == 6 / 5 and float(dens_golden["co_631g"]["scs_c_ss"]) == 1 / 3


@pytest.mark.parametrize("tag", list(SYSTEMS))
def test_restatement_against_the_golden(dens_golden, tag):
    g = dens_golden[tag]
    _, shells, aos = system(tag)
    E = mr.dense_eri(aos, shells)
    C, eps, nocc = g["C"], g["eps"], int(g["n_occ"])
    gmo = mr.mo_integrals(E, C)
    for m in METHODS:
        c_os, c_ss = float(g[f"{m}_c_os"]), float(g[f"{m}_c_ss"])
        for kind in ("unrelaxed", "relaxed"):
            r = mr.mp2_density(E, C, eps, nocc, 0, kind == "relaxed", c_os, c_ss, g=gmo)
            d_mo = np.abs(r["P_mo"] - g[f"{m}_P_mo_{kind}"]).max()
            d_ao = np.abs(r["P_ao"] - g[f"{m}_P_ao_{kind}"]).max()
            d_z = np.abs(r["z"] - g[f"{m}_z"]).max() if kind == "relaxed" else 0.0
            d_e = max(abs(r["E_OS"] - float(g["E_OS"])), abs(r["E_SS"] - float(g["E_SS"])))
            print(f"\n[{tag} {m} {kind}] dP_mo {d_mo:.1e} dP_ao {d_ao:.1e} dz {d_z:.1e} dE {d_e:.1e}")
            assert d_mo < TOL and d_ao < TOL and d_z < TOL and d_e < TOL
            assert abs(np.trace(r["P_mo"]) - 2 * nocc) < 1e-11                      # tr P_mo = the number of electrons
            assert abs(np.sum(r["P_ao"] * g["S"]) - 2 * nocc) < 1e-11
            assert np.abs(r["P_mo"] - r["P_mo"].T).max() < 1e-14 and np.abs(r["P_ao"] - r["P_ao"].T).max() < 1e-13
            occ, orb = mr.natural_orbitals(r["P_ao"], g["X"])
            want = g[f"{m}_occ"] if kind == "relaxed" else g[f"{m}_occ_unrelaxed"]
            assert np.abs(occ - want).max() < 1e-11 and np.all(np.diff(occ) <= 1e-14)
            assert np.abs(orb.T @ g["S"] @ orb - np.eye(len(eps))).max() < 1e-11
            mu = g[f"{m}_dipole"] if kind == "relaxed" else g[f"{m}_dipole_unrelaxed"]
            assert abs(-np.sum(r["P_ao"] * g["dipz"]) - mu[2]) < 1e-11 and abs(mu[0] - (mu[1] + mu[2])) < 1e-14
        if nocc > 1:                                                               # (o = v = 1: z is zero by symmetry)
            assert np.abs(g[f"{m}_P_mo_relaxed"] - g[f"{m}_P_mo_unrelaxed"]).max() > 1e-3


def test_field_derivative_and_the_bound_of_the_gpu_test():
    """Independent of the reference program: for CO/6-31G, Tr(P_relaxed D_z) is dE/dF_z of E_RHF + E_MP2 (oracle/scf_oracle.py's cycle
    at EXTREME thresholds with F D_z in the core Hamiltonian, the four-point stencil).  The stencil at h = 0.004 and at h / 2 gives
    -0.08567957245 and -0.08567956854; ten times their difference, 3.9e-8, is the bound of tests/test_gpu_mp2_density.py, which this
    test derives again.  The relaxed density meets it, the unrelaxed one (+0.1509) does not."""
    from oracle import scf_oracle as so
    h, bound = 0.004, 3.9e-8
    atoms, shells, aos = system("co_631g")
    sd = mr.field_system(atoms, shells, aos)
    cache = {}

    def E(F):
        key = round(F / (h / 2))
        if key not in cache:
            cache[key] = mr.cpu_field_energy(sd, 7, F)
        return cache[key]
    d_h, d_half = mr.stencil(E, h), mr.stencil(E, h / 2)
    print(f"\n[co_631g] stencil at h {d_h:.11f} at h / 2 {d_half:.11f} ten times the difference {10 * abs(d_h - d_half):.2e}")
    assert abs(10 * abs(d_h - d_half) / bound - 1) < 0.05
    P0, E0 = so.core_guess(sd["T"], sd["V"], sd["X"], 7)
    r = so.run_rhf(sd["S"], sd["T"], sd["V"], sd["E"], sd["X"], P0, E0, 7, sd["V_NN"], sd["ranges"], conv="extreme")
    tr = {rel: float(np.sum(mr.mp2_density(sd["E"], r["C"], r["epsilons"], 7, 0, rel)["P_ao"] * sd["Dz"])) for rel in (True, False)}
    assert abs(tr[True] - d_h) < bound and abs(tr[True] - d_half) < bound
    assert not abs(tr[False] - d_h) < bound and abs(tr[False] - 0.1509) < 1e-4


def test_frozen_core_and_refusal(dens_golden):
    g = dens_golden["co_631g"]
    _, shells, aos = system("co_631g")
    E = mr.dense_eri(aos, shells)
    C, eps, nocc = g["C"], g["eps"], int(g["n_occ"])
    r = mr.mp2_density(E, C, eps, nocc, 1)
    assert abs(np.trace(r["P_mo"]) - 2 * nocc) < 1e-11
    assert np.all(r["P_mo"][0, 1:] == 0) and r["P_mo"][0, 0] == 2.0               # the frozen orbital keeps the reference determinant's 2
    with pytest.raises(ValueError):
        mr.mp2_density(E, C, eps, nocc, 1, relaxed=True)


# ---- the cases of tests/test_gpu_mp2_density_shapes.py on a dense tensor, and what makes their bounds hold -------------------------------
WIDTHS = (1, 2, 7, 8, 12, 16)              # N2/cc-pVTZ, random orbitals: the occupied widths
SMALL_O = (7, 8, 9)                        # N2/STO-3G (N = 10): v = 3, 2, 1
SMALL_SEED = {7: 47, 8: 48, 9: 49}         # seeds of the random C at N = 10 (40 + o, as test_small_virtual_spaces of the triples)
FROZEN = ((12, 5), (12, 11))               # (width, n_frozen), unrelaxed only
SCS = (6 / 5, 1 / 3)
DEVICE_BOUND = 1e-12                       # |device - checker| <= 1e-12 S per element on the GPU


def width_orbitals(N, width):
    """_random_orbitals(N, 30 + width) of tests/test_gpu_mp3.py with the virtual energies 1 Eh higher (shifted_random_orbitals of
    tests/test_gpu_cis.py): orthonormal columns without any symmetry"""
    from test_gpu_mp3 import _random_orbitals
    C, eps = _random_orbitals(N, 30 + width)
    eps = eps.copy()
    eps[width:] += 1.0
    return C, eps


def small_orbitals(N, o):
    """the orbitals of test_small_virtual_spaces (tests/test_gpu_triples.py): occupied -20 ... -11, virtual 0.3 ... 2.0"""
    C = np.linalg.qr(np.random.default_rng(SMALL_SEED[o]).standard_normal((N, N)))[0]
    return C, np.concatenate([-np.linspace(20.0, 11.0, o), np.linspace(0.3, 2.0, N - o)])


def dense_cases():
    """(label, tensor tag, C, eps, n_occ, n_frozen, relaxed) of every case the GPU file runs on a dense tensor"""
    out = []
    for w in WIDTHS:
        out.append((f"tz width {w}", "n2_ccpvtz", *width_orbitals(60, w), w, 0, True))
    for o in SMALL_O:
        out.append((f"min o {o}", "n2_sto3g", *small_orbitals(10, o), o, 0, True))
    for w, nf in FROZEN:
        out.append((f"tz width {w} frozen {nf}", "n2_ccpvtz", *width_orbitals(60, w), w, nf, False))
    return out


def window_blocks(g, n_occ, n_frozen, relaxed=True):
    """(ia|jb), (ij|ab), (ji|kb), (ia|bc) of the window from the full MO tensor g"""
    o, v = slice(n_frozen, n_occ), slice(n_occ, g.shape[0])
    return (g[o, v, o, v],) + ((g[o, o, v, v], g[o, o, o, v], g[o, v, v, v]) if relaxed else (None, None, None))


@pytest.fixture(scope="module")
def dense_mo():
    """the float64 MO tensor of every dense case, formed once"""
    from test_gpu_mp3 import _system
    E, out = {}, {}
    for label, tag, C, eps, nocc, nf, relaxed in dense_cases():
        if tag not in E:
            shells, aos = _system(tag)
            E[tag] = mr.dense_eri(aos, shells)
        out[label] = (E[tag], mr.mo_integrals(E[tag], C), C, eps, nocc, nf, relaxed)
    return out


def _ratios(a, b, keys=(("P_oo", "S_oo"), ("P_vv", "S_vv"), ("L", "S_L"), ("E_OS", "S_E_OS"), ("E_SS", "S_E_SS"))):
    """worst |a - b| / S per quantity, S from a"""
    out = {}
    for k, s in keys:
        if a.get(k) is None:
            continue
        d = np.abs(np.asarray(a[k], dtype=np.longdouble) - np.asarray(b[k], dtype=np.longdouble)).astype(np.float64)
        out[k] = float(np.max(d / np.asarray(a[s], dtype=np.float64)))
    return out


def _with_blocks(r, no):
    """P_oo and P_vv (without the reference determinant's 2) next to the other outputs of mp2_density_from_blocks"""
    r = dict(r)
    r["P_oo"], r["P_vv"] = r["P2"][:no, :no], r["P2"][no:, no:]
    return r


def test_existing_outputs_keep_their_bits(dens_golden):
    """mp2_density returns what it returned before the sums of magnitudes came: the statements of the module as they stood, inline"""
    g = dens_golden["co_631g"]
    _, shells, aos = system("co_631g")
    E, C, eps, nocc = mr.dense_eri(aos, shells), g["C"], g["eps"], int(g["n_occ"])
    gmo = mr.mo_integrals(E, C)
    r = mr.mp2_density(E, C, eps, nocc, 0, True, *SCS, g=gmo)
    o, v = slice(0, nocc), slice(nocc, len(eps))
    G = gmo[o, v, o, v]
    Gx = G.transpose(0, 3, 2, 1)
    D = eps[o][:, None, None, None] + eps[o][None, None, :, None] - eps[v][None, :, None, None] - eps[v][None, None, None, :]
    w = SCS[0] * 2.0 * G / D + SCS[1] * 2.0 * (G - Gx) / D
    tos, tss = -2.0 * G / D, (G - Gx) / D
    P2 = np.zeros_like(r["P_mo"])
    for c, t, f in ((SCS[0], tos, 0.5), (SCS[1], tss, 1.0)):
        P2[o, o] += -f * c * np.einsum("kaib,kajb->ij", t, t, optimize=True)
        P2[v, v] += f * c * np.einsum("ibjc,iajc->ab", t, t, optimize=True)
    L = 2.0 * np.einsum("ibjc,abjc->ia", w, gmo[v, v, o, v], optimize=True)
    L -= 2.0 * np.einsum("jakb,jikb->ia", w, gmo[o, o, o, v], optimize=True)
    L += (4.0 * np.einsum("pqrs,rs->pq", gmo, P2, optimize=True) - 2.0 * np.einsum("prqs,rs->pq", gmo, P2, optimize=True))[o, v]
    assert np.array_equal(r["L"], L) and r["E_OS"] == float(np.sum(G * G / D)) and r["E_SS"] == float(np.sum(G * (G - Gx) / D))
    assert np.array_equal(r["P_mo"][o, o], P2[o, o] + 2.0 * np.eye(nocc)) and np.array_equal(r["P_mo"][v, v], P2[v, v])
    assert np.array_equal(r["P_mo"][o, v], 0.5 * r["z"]) and np.abs(r["z"] - g["scs_z"]).max() < TOL
    assert set(r) >= {"S_oo", "S_vv", "S_L", "S_M", "S_E_OS", "S_E_SS", "lambda_min", "norm2"}
    # every magnitude sum dominates its value, and A + B's spectrum is that of the matrix the solve used
    assert np.all(r["S_oo"] >= np.abs(P2[o, o])) and np.all(r["S_vv"] >= np.abs(P2[v, v])) and np.all(r["S_L"] >= np.abs(L))
    assert r["S_E_OS"] >= abs(r["E_OS"]) and r["S_E_SS"] >= abs(r["E_SS"])
    assert abs(r["norm2"] / r["lambda_min"] / r["cond"] - 1) < 1e-10


@pytest.mark.parametrize("kind", ["unrelaxed", "relaxed"])
def test_from_blocks_against_dense(golden, kind):
    """N2/cc-pVDZ, random orthonormal orbitals, SCS weights: the block restatement gives the dense one's P, L, z and energies within
    1e-13 S per element (z: within 1e-13 S_L carried through the solve), the same S to 1e-13, and the dense J/K of the dense one
    never formed."""
    from test_gpu_mp3 import _random_orbitals, _system
    shells, aos = _system("n2_ccpvdz")
    E = mr.dense_eri(aos, shells)
    N, nocc, relaxed = E.shape[0], 7, kind == "relaxed"
    C, eps = _random_orbitals(N, 37)
    eps = eps.copy()
    eps[nocc:] += 1.0
    gmo = mr.mo_integrals(E, C)
    d = mr.mp2_density(E, C, eps, nocc, 0, relaxed, *SCS, g=gmo)
    b = _with_blocks(mr.mp2_density_from_blocks(eps[:nocc], eps[nocc:], *window_blocks(gmo, nocc, 0, relaxed), relaxed, *SCS), nocc)
    d["P_oo"], d["P_vv"] = d["P_mo"][:nocc, :nocc] - 2.0 * np.eye(nocc), d["P_mo"][nocc:, nocc:]
    worst = _ratios(d, b)
    print(f"\n[n2_ccpvdz random, {kind}] worst |blocks - dense| / S {worst}")
    assert all(x <= 1e-13 for x in worst.values()), worst
    # the +2 of the occupied diagonal is rounded in one ulp of 2
    assert np.abs(b["P_mo"][:nocc, :nocc] - d["P_mo"][:nocc, :nocc]).max() <= 1e-13 * d["S_oo"].max() + 2.0 ** -51
    for k in ("S_oo", "S_vv", "S_L", "S_M"):
        assert (d[k] is None and b[k] is None) or np.abs(d[k] - b[k]).max() <= 1e-13 * np.abs(d[k]).max(), k
    if relaxed:
        dz = np.abs(d["z"] - b["z"]).max()
        bound = z_bound(d, 1e-13, nocc * (N - nocc))
        print(f"[n2_ccpvdz random] |dz| {dz:.1e} bound {bound:.1e} lambda_min {d['lambda_min']:.3f} cond {d['cond']:.1f}")
        assert dz <= bound and np.array_equal(b["P_mo"][:nocc, nocc:], 0.5 * b["z"])
    else:
        assert b["L"] is None and b["z"] is None and not b["P_mo"][:nocc, nocc:].any()


def z_bound(ref, unit, dim):
    """max |dz| of a solve whose right-hand side and matrix are off by unit S_L and unit S_M element by element, first order:
    [ ||unit S_L||_2 + (||unit S_M||_F + dim 2^-53 ||M||_2) ||z||_2 ] / lambda_min, the last matrix term a backward-stable Cholesky"""
    return float((np.linalg.norm(unit * ref["S_L"]) + (np.linalg.norm(unit * ref["S_M"]) + dim * 2.0 ** -53 * ref["norm2"]) * np.linalg.norm(ref["z"]))
                 / ref["lambda_min"])


def test_the_reference_stays_inside_the_device_bound(dense_mo):
    """Every dense case of the GPU file: the checker's contractions in float64 against the same in np.longdouble on the same float64 MO
    integrals differ by at most a tenth of the device bound, 1e-13 S, element by element.  Measured, the worst over the cases: 5.1e-15
    (P_oo), 1.0e-15 (P_vv), 4.5e-16 (L), 1.5e-16 (energies)."""
    bad = []
    for label, (E, gmo, C, eps, nocc, nf, relaxed) in dense_mo.items():
        args = (eps[nf:nocc], eps[nocc:], *window_blocks(gmo, nocc, nf, relaxed), relaxed, *SCS)
        a = _with_blocks(mr.mp2_density_from_blocks(*args), nocc - nf)
        b = _with_blocks(mr.mp2_density_from_blocks(*args, dtype=np.longdouble), nocc - nf)
        worst = _ratios(a, b)
        print(f"\n[{label}] worst |float64 - longdouble| / S {({k: f'{x:.1e}' for k, x in worst.items()})}")
        if not all(x <= 0.1 * DEVICE_BOUND for x in worst.values()):
            bad.append((label, worst))
    assert not bad, bad


def test_the_inputs_are_well_posed(dense_mo):
    """Every dense case: every denominator D < 0; relaxed ones: lambda_min(A + B) > 1.0 and cond(A + B) < 50."""
    bad = []
    for label, (E, gmo, C, eps, nocc, nf, relaxed) in dense_mo.items():
        r = mr.mp2_density_from_blocks(eps[nf:nocc], eps[nocc:], *window_blocks(gmo, nocc, nf, relaxed), relaxed, *SCS)
        line = f"\n[{label}] max D {r['D_max']:.3f}"
        ok = r["D_max"] < 0
        if relaxed:
            line += f" lambda_min {r['lambda_min']:.3f} cond {r['cond']:.1f} max|z| {np.abs(r['z']).max():.2e} z bound {z_bound(r, DEVICE_BOUND, r['z'].size):.1e}"
            ok = ok and r["lambda_min"] > 1.0 and r["cond"] < 50
        print(line)
        if not ok:
            bad.append(label)
    assert not bad, bad
