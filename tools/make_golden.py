#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ from the REAL reference, in the build container.

What runs here (needs /root/reference and oracle/_ref built by oracle/build_ref.sh):
  * the compiled, unmodified reference integral engine (tuna_integrals/tuna_integral.pyx);
  * the reference's own SCF module TUNA/tuna_scf.py, executed from its source text.  Under this
    container's Python 3.10 exactly one statement of that file does not parse (a PEP-701 nested-quote
    f-string inside a log() call, tuna_scf.py:1319); that single logging line is replaced by `pass`.
    Its imports (tuna_util, tuna_molecule, tuna_calc, tuna_dft, tuna_xc) are satisfied by tiny stand-in
    modules that provide only logging no-ops, `symmetrise` (tuna_util.py:748-764, one line) and an
    `Output` record; no numerical routine is stubbed;
  * the literal spherical-harmonic tables and `calculate_orthogonalisation_matrix`, executed from the
    text of tuna_kernel.py:554-623 and :756-816.
Only DATA (inputs and expected outputs) is written to tests/golden/; no reference source is stored.
"""
from __future__ import annotations

import ast
import os
import sys
import types

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
REF = os.environ.get("TUNA_REFERENCE", "/root/reference")
GOLD = os.path.join(ROOT, "tests", "golden")

from oracle import oracle as orc  # noqa: E402
from tuna_amd import molecule as mol  # noqa: E402


# --------------------------------------------------------------------------------------------
# loading pieces of the reference from text
# --------------------------------------------------------------------------------------------

def _stub_modules():
    tu = types.ModuleType("tuna_util")
    tu.symmetrise = lambda m: (1 / 2) * (m + m.T)          # tuna_util.py:762
    tu.log = lambda *a, **k: None
    tu.warning = lambda *a, **k: None
    tu.log_big_spacer = lambda *a, **k: None
    tu.log_spacer = lambda *a, **k: None
    tu.timer = lambda *a, **k: None

    def error(msg):
        raise RuntimeError(msg)
    tu.error = error

    class Output:
        def __init__(self, *args):
            names = ["energy", "kinetic_energy", "nuclear_electron_energy", "coulomb_energy", "exchange_energy",
                     "correlation_energy", "electric_field_energy", "electric_field_gradient_energy", "P",
                     "P_alpha", "P_beta", "S", "X", "molecular_orbitals", "molecular_orbitals_alpha",
                     "molecular_orbitals_beta", "epsilons", "epsilons_alpha", "epsilons_beta", "density",
                     "alpha_density", "beta_density", "F_alpha", "F_beta", "T", "V_NE", "integrals"]
            for n, a in zip(names, args):
                setattr(self, n, a)
    tu.Output = Output
    tu.exchange_correlation_functionals = {}
    tu.Integrals = object
    mods = {"tuna_util": tu}
    for name, attr in (("tuna_molecule", "Molecule"), ("tuna_calc", "Calculation")):
        m = types.ModuleType(name)
        setattr(m, attr, object)
        mods[name] = m
    mods["tuna_dft"] = types.ModuleType("tuna_dft")
    mods["tuna_xc"] = types.ModuleType("tuna_xc")
    return mods


def _parseable_lines(path):
    lines = open(path).read().split("\n")
    patched = []
    for _ in range(200):
        try:
            ast.parse("\n".join(lines))
            break
        except SyntaxError as e:
            ln = e.lineno - 1
            indent = len(lines[ln]) - len(lines[ln].lstrip())
            patched.append(e.lineno)
            lines[ln] = " " * indent + "pass"
    return lines, patched


def load_reference_scf():
    lines, patched = _parseable_lines(os.path.join(REF, "TUNA", "tuna_scf.py"))
    assert patched == [1319], f"unexpected unparsable lines in tuna_scf.py: {patched}"
    saved = {k: sys.modules.get(k) for k in _stub_modules()}
    sys.modules.update(_stub_modules())
    mod = types.ModuleType("ref_tuna_scf")
    try:
        exec(compile("\n".join(lines), "tuna_scf.py", "exec"), mod.__dict__)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def load_reference_kernel_bits():
    """U_S..U_H tables and calculate_orthogonalisation_matrix from tuna_kernel.py text."""
    src = open(os.path.join(REF, "TUNA", "tuna_kernel.py")).read().split("\n")
    ns = {"np": np}
    exec("\n".join(l[4:] if l.startswith("    ") else l for l in src[553:623]), ns)
    blocks = {L: np.array(ns[k]) for L, k in enumerate(["U_S", "U_P", "U_D", "U_F", "U_G", "U_H"])}
    stubs = _stub_modules()["tuna_util"]
    ns2 = {"np": np, "ndarray": np.ndarray, "Calculation": object, "symmetrise": stubs.symmetrise,
           "log": stubs.log, "timer": stubs.timer, "error": stubs.error}
    exec("\n".join(src[755:816]), ns2)
    return blocks, ns2["calculate_orthogonalisation_matrix"]


# --------------------------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------------------------

def system(symbols, R_bohr, basis, decontract=False):
    atoms = mol.make_atoms(symbols, R_bohr)
    shells = mol.build_shells(atoms, basis, decontract)
    return atoms, shells, mol.expand_cartesian_aos(shells)


def reference_U(shells, blocks):
    from scipy.linalg import block_diag
    return block_diag(*[blocks[s.L] for s in shells])


def to_spherical(U, M):
    return U @ M @ U.T


def eri_to_spherical(U, E):
    E = np.tensordot(U, E, axes=(1, 0))                    # a jkl
    E = np.tensordot(U, E, axes=(1, 1)).transpose(1, 0, 2, 3)
    E = np.tensordot(U, E, axes=(1, 2)).transpose(1, 2, 0, 3)
    E = np.tensordot(U, E, axes=(1, 3)).transpose(1, 2, 3, 0)
    return np.ascontiguousarray(E)


def com_z(atoms):
    # only used as the dipole origin; masses are irrelevant for parity as long as both sides use the same point
    return 0.5 * atoms[-1].origin[2] if len(atoms) == 2 else 0.0


def one_e_and_eri(atoms, aos):
    xyz = [a.origin for a in atoms]
    chg = [float(a.charge) for a in atoms]
    S, T, V, D, Q = orc.ref_one_electron(aos, xyz, chg, [0.0, 0.0, com_z(atoms)])
    E = orc.ref_eri(aos)
    return S, T, V, D, Q, E


def sample_indices(n, count, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, size=(count, 4)).astype(np.int32)


class Calc:  # duck-typed Calculation (fields read by tuna_scf.py)
    def __init__(self, conv, damping=True, diis=True, max_iter=100):
        self.reference = "RHF"
        self.DFT_calculation = False
        self.HFX_prop = 1
        self.DFX_prop = 0
        self.DFC_prop = 0
        self.DIIS = diis
        self.max_DIIS_matrices = 6
        self.damping = damping
        self.damping_factor = None
        self.max_damping = 0.7
        self.max_iter = max_iter
        self.SCF_conv = conv
        self.method = types.SimpleNamespace(name="HF")


class Ints:
    def __init__(self, S, T, V, ERI):
        self.S, self.T, self.V_NE, self.ERI_AO = S, T, V, ERI
        self.F = np.zeros_like(S)
        self.G = np.zeros_like(S)
        self.H_core = T + V
        self.one_electron_integrals = (S, T, V, None)


CONV = {
    "medium": {"delta_E": 0.0000001, "max_DP": 0.000001, "RMS_DP": 0.0000001, "commutator": 0.00001, "name": "medium"},
    "extreme": {"delta_E": 0.00000000001, "max_DP": 0.0000000001, "RMS_DP": 0.00000000001, "commutator": 0.000000001, "name": "extreme"},
}


def run_reference_uhf(scf, ortho, atoms, shells, S, T, V, ERI, n_alpha, n_beta, conv="extreme", damping=True):
    """The reference's UNRESTRICTED cycle (scf:1165-1281) from a core-Hamiltonian guess with n_alpha / n_beta occupations."""
    X, smallest, S_inv = ortho(S, None, True)
    eps0, C0 = scf.diagonalise_Fock_matrix(T + V, X)
    Pa0 = scf.construct_density_matrix(C0, n_alpha, 1)
    Pb0 = scf.construct_density_matrix(C0, n_beta, 1)
    E0 = float(np.einsum("mn,mn->", T + V, Pa0 + Pb0))
    n_sph = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    molecule = types.SimpleNamespace(n_doubly_occ=n_beta, partition_ranges=n_sph, atoms=atoms, n_electrons=n_alpha + n_beta,
                                     n_alpha=n_alpha, n_beta=n_beta)
    table = []
    orig = scf.format_output_line

    def rec(E_total, delta_E, max_DP, RMS_DP, damping_factor, step, commutator, calculation, silent=False):
        table.append([step, E_total, delta_E, RMS_DP, max_DP, commutator, float(damping_factor)])
    scf.format_output_line = rec
    try:
        V_NN = mol.nuclear_repulsion(atoms)
        calc = Calc(CONV[conv], damping=damping)
        calc.reference = "UHF"
        out = scf.run_self_consistent_field_cycle(molecule, calc, Ints(S, T, V, ERI), V_NN, X,
                                                  (Pa0 + Pb0, Pa0, Pb0, E0), (None, None, None, None), True)
    finally:
        scf.format_output_line = orig
    return dict(table=np.array(table), energy=out.energy, epsilons_alpha=out.epsilons_alpha, epsilons_beta=out.epsilons_beta,
                P_alpha=out.P_alpha, P_beta=out.P_beta, E0=E0, V_NN=V_NN,
                components=np.array([out.kinetic_energy, out.nuclear_electron_energy, out.coulomb_energy, out.exchange_energy]))


def load_reference_ao_to_mo():
    """transform_ERI_AO_to_MO (tuna_ci.py:204-255) and build_doubles_epsilons_tensor (tuna_ci.py:304-334) from source text."""
    src = open(os.path.join(REF, "TUNA", "tuna_ci.py")).read()
    tree = ast.parse(src)
    stubs = _stub_modules()["tuna_util"]
    ns = {"np": np, "ndarray": np.ndarray, "Calculation": object, "log": stubs.log, "timer": stubs.timer, "error": stubs.error}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("transform_ERI_AO_to_MO", "build_doubles_epsilons_tensor"):
            exec(compile(ast.Module([node], []), "tuna_ci.py", "exec"), ns)
    return ns["transform_ERI_AO_to_MO"], ns["build_doubles_epsilons_tensor"]


def make_mp2_golden(scf, blocks, ortho):
    """Config 5: RMP2 on converged RHF orbitals -- the reference's own AO->MO transformation and the energy expressions of
    run_restricted_MP2 (tuna_mp.py:874-890: physicists' transpose, [o,o,v,v] slice, E_OS and E_SS einsums)."""
    ao_to_mo, doubles_eps = load_reference_ao_to_mo()
    out = {}
    for tag, (sym, R, basis, nocc) in {
        "n2_sto3g": (["N", "N"], mol.angstrom_to_bohr(1.0977), "STO-3G", 7),
        "n2_ccpvdz": (["N", "N"], mol.angstrom_to_bohr(1.0977), "cc-pVDZ", 7),
        "c5_n2_ccpvtz": (["N", "N"], mol.angstrom_to_bohr(1.0977), "cc-pVTZ", 7),
        "co_631g": (["C", "O"], mol.angstrom_to_bohr(1.128), "6-31G", 7),
    }.items():
        atoms, shells, aos = system(sym, R, basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        U = reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V), eri_to_spherical(U, E)
        r = run_reference_scf(scf, ortho, atoms, shells, Ss, Ts_, Vs, Es, nocc, "extreme", tag.startswith("co"))   # CO needs damping
        C, eps = r["C"], r["epsilons"]
        ERI_MO = ao_to_mo(Es, C, None, True)
        o, v = slice(0, nocc), slice(nocc, len(eps))
        e_ijab = doubles_eps(eps, eps, o, o, v, v)
        g = ERI_MO.transpose(0, 2, 1, 3)[o, o, v, v]
        E_OS = np.einsum("ijab,ijab,ijab->", g, g, e_ijab, optimize=True)
        E_SS = np.einsum("ijab,ijab,ijab->", g, g - g.swapaxes(2, 3), e_ijab, optimize=True)
        idx = sample_indices(len(eps), 5000, 9)
        out[tag] = dict(C=C, eps=eps, E_SCF=r["energy"], E_OS=E_OS, E_SS=E_SS, n_occ=nocc, mo_idx=idx,
                        mo_val=ERI_MO[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]])
        print("MP2", tag, len(eps), "E_SCF", r["energy"], "E_MP2", E_OS + E_SS, "OS", E_OS, "SS", E_SS)
    np.savez_compressed(os.path.join(GOLD, "mp2_systems.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


def make_sad_golden(scf, blocks, ortho):
    """The reference's DEFAULT single-point path: superposition-of-atomic-densities guess (tuna_guess.py functions executed from
    source text, atomic densities from the literal table of tuna_util.py) followed by the reference SCF with default keywords
    (DIIS 6 + dynamic damping) at the default "medium" thresholds and at "extreme"."""
    import json
    src = open(os.path.join(REF, "TUNA", "tuna_guess.py")).read()
    tree = ast.parse(src)
    from scipy.linalg import block_diag
    ns = {"np": np, "ndarray": np.ndarray, "block_diag": block_diag, "Atom": object}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("project_density_matrix", "form_minimal_basis_superposition_density"):
            exec(compile(ast.Module([node], []), "tuna_guess.py", "exec"), ns)
    dens = {k: (None if v["density"] is None else np.array(v["density"])) for k, v in
            json.load(open(os.path.join(ROOT, "tuna_amd", "data", "atomic_data.json"))).items()}
    ints_ref = orc.ref_engine()
    out = {}
    for tag, (sym, R, basis, nocc) in {
        "c1_h2_sto3g": (["H", "H"], mol.angstrom_to_bohr(0.74), "STO-3G", 1),
        "n2_ccpvdz": (["N", "N"], mol.angstrom_to_bohr(1.0977), "cc-pVDZ", 7),
        "c2_n2_ccpvtz": (["N", "N"], mol.angstrom_to_bohr(1.0977), "cc-pVTZ", 7),
        "c4_co_def2tzvp": (["C", "O"], mol.angstrom_to_bohr(1.128), "def2-TZVP", 7),
        "ne_631g": (["NE"], None, "6-31G", 5),
    }.items():
        atoms, shells, aos = system(sym, R, basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        U = reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V), eri_to_spherical(U, E)
        X, smallest, S_inv = ortho(Ss, None, True)
        ref_atoms = [types.SimpleNamespace(density=dens[a.symbol]) for a in atoms]
        P_min = ns["form_minimal_basis_superposition_density"](ref_atoms)
        _, _, aos_min = system(sym, R, "STO-3G")
        S_cross = np.asarray(ints_ref.calculate_cross_basis_overlap_matrix(aos.n, aos_min.n, orc.ref_basis_list(aos), orc.ref_basis_list(aos_min), 4))
        P_spin = ns["project_density_matrix"](P_min, S_cross, S_inv, U)
        Pa = P_spin * (nocc / np.trace(P_spin @ Ss))                      # clean_density_matrix, tuna_dft.py:35-41
        P0 = Pa + Pa
        E0 = float(np.einsum("mn,mn->", Ts_ + Vs, P0, optimize=True))
        n_sph = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
        d = dict(P_guess=P0, E_guess=E0)
        for conv in ("medium", "extreme"):
            molecule = types.SimpleNamespace(n_doubly_occ=nocc, partition_ranges=n_sph, atoms=atoms, n_electrons=2 * nocc, n_alpha=nocc, n_beta=nocc)
            table = []
            orig = scf.format_output_line

            def rec(E_total, delta_E, max_DP, RMS_DP, damping_factor, step, commutator, calculation, silent=False):
                table.append([step, E_total, delta_E, RMS_DP, max_DP, commutator, float(damping_factor)])
            scf.format_output_line = rec
            try:
                o = scf.run_self_consistent_field_cycle(molecule, Calc(CONV[conv], damping=True), Ints(Ss, Ts_, Vs, Es), mol.nuclear_repulsion(atoms), X,
                                                        (P0, Pa, Pa, E0), (None, None, None, None), True)
            finally:
                scf.format_output_line = orig
            d[f"table_{conv}"] = np.array(table)
            d[f"energy_{conv}"] = o.energy
        out[tag] = d
        print("SAD", tag, aos.n, "E_guess", E0, "E", d["energy_medium"], d["energy_extreme"], "iters", len(d["table_medium"]), len(d["table_extreme"]))
    np.savez_compressed(os.path.join(GOLD, "sad_default_runs.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


def load_reference_dft():
    """tuna_xc.py (parses as is) and tuna_dft.py (one PEP-701 log line patched to `pass`), executed from source text against
    stand-in modules that carry only logging no-ops, `symmetrise`, `check` and the three numerical floors of
    tuna_util.constants (density_floor 1e-23, sigma_floor 1e-46, exponent_ceiling 600: tuna_util.py:95-99)."""
    stubs = _stub_modules()
    tu = stubs["tuna_util"]
    tu.constants = types.SimpleNamespace(density_floor=1e-23, exponent_ceiling=600, sigma_floor=1e-23 ** 2)

    def check(assertion, message):
        if not assertion:
            raise RuntimeError(message)
    tu.check = check
    saved = {k: sys.modules.get(k) for k in list(stubs) + ["tuna_xc"]}
    sys.modules.update(stubs)
    try:
        xc = types.ModuleType("tuna_xc")
        exec(compile(open(os.path.join(REF, "TUNA", "tuna_xc.py")).read(), "tuna_xc.py", "exec"), xc.__dict__)
        sys.modules["tuna_xc"] = xc
        lines, patched = _parseable_lines(os.path.join(REF, "TUNA", "tuna_dft.py"))
        dft = types.ModuleType("tuna_dft")
        exec(compile("\n".join(lines), "tuna_dft.py", "exec"), dft.__dict__)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return xc, dft, patched


DFT_FUNCTIONAL_SWEEP = {        # one small system per functional of tuna_amd.dft.FUNCTIONALS that dft_systems.npz does not exercise
    "lih_hfs_sto3g": (["LI", "H"], 1.595, "STO-3G", 2, "HFS", "loose"),
    "lih_svwn3_sto3g": (["LI", "H"], 1.595, "STO-3G", 2, "SVWN3", "loose"),
    "hf_hfb_631g": (["F", "H"], 0.917, "6-31G", 5, "HFB", "loose"),
    "hf_bvwn_631g": (["F", "H"], 0.917, "6-31G", 5, "BVWN", "loose"),
    "lih_bvwn3_sto3g": (["LI", "H"], 1.595, "STO-3G", 2, "BVWN3", "loose"),
    "hf_bhlyp_631g": (["F", "H"], 0.917, "6-31G", 5, "BHLYP", "loose"),
    "hf_b1lyp_631g": (["F", "H"], 0.917, "6-31G", 5, "B1LYP", "loose"),
    "lih_slyp_sto3g": (["LI", "H"], 1.595, "STO-3G", 2, "SLYP", "loose"),
}


def make_dft_golden(scf, blocks, ortho, systems=None, outfile="dft_systems.npz"):
    """BASELINE config 4 (CO B3LYP/def2-TZVP, "medium" grid) and smaller Kohn-Sham cases with the reference's own grid, basis-on-grid,
    density, functional and V_XC code, and its SCF loop with DFT switched on.  `systems` (tag -> (symbols, R in bohr, basis, n_occ,
    method, grid)) and `outfile` select another set (--dft-sweep-only: DFT_FUNCTIONAL_SWEEP -> dft_functionals.npz)."""
    import json
    xc, dft, patched = load_reference_dft()
    print("tuna_dft.py lines patched:", patched)
    scf.dft, scf.xc = dft, xc                                       # tuna_scf.py does `import tuna_dft as dft`, `import tuna_xc as xc`
    adata = json.load(open(os.path.join(ROOT, "tuna_amd", "data", "atomic_data.json")))
    GRID = {"loose": (3, 0.7), "medium": (4, 0.9), "tight": (5, 1.0)}            # tuna_util.py:129-137
    # (x functional, c functional, DFX, HFX, DFC, class): the rows of the reference's table, tuna_util.py:1445-1475
    FUN = {"B3LYP": ("B3", "3P", 0.80, 0.20, 1.0, "GGA"), "BLYP": ("B", "LYP", 1.0, 0.0, 1.0, "GGA"), "LDA": ("S", "VWN5", 1.0, 0.0, 1.0, "LDA"),
           "B3LYP/G": ("B3", "3P", 0.80, 0.20, 1.0, "GGA"), "HFS": ("S", None, 1.0, 0.0, 0.0, "LDA"), "SVWN3": ("S", "VWN3", 1.0, 0.0, 1.0, "LDA"),
           "HFB": ("B", None, 1.0, 0.0, 0.0, "GGA"), "BVWN": ("B", "VWN5", 1.0, 0.0, 1.0, "GGA"), "BVWN3": ("B", "VWN3", 1.0, 0.0, 1.0, "GGA"),
           "BHLYP": ("B", "LYP", 0.50, 0.50, 1.0, "GGA"), "B1LYP": ("B", "LYP", 0.75, 0.25, 1.0, "GGA"), "SLYP": ("S", "LYP", 1.0, 0.0, 1.0, "GGA")}
    out = {}
    if systems is None:
        systems = {
            "h2_lda_sto3g": (["H", "H"], mol.angstrom_to_bohr(0.74), "STO-3G", 1, "LDA", "loose"),
            "n2_blyp_631g": (["N", "N"], mol.angstrom_to_bohr(1.0977), "6-31G", 7, "BLYP", "loose"),
            "co_b3lyp_631g": (["C", "O"], mol.angstrom_to_bohr(1.128), "6-31G", 7, "B3LYP", "medium"),
            "co_b3lypg_ccpvdz": (["C", "O"], mol.angstrom_to_bohr(1.128), "cc-pVDZ", 7, "B3LYP/G", "loose"),
            "c4_co_b3lyp_def2tzvp": (["C", "O"], mol.angstrom_to_bohr(1.128), "def2-TZVP", 7, "B3LYP", "medium"),
        }
    for tag, (sym, R, basis, nocc, method, grid) in systems.items():
        atoms, shells, aos = system(sym, R, basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        U = reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V), eri_to_spherical(U, E)
        X, smallest, S_inv = ortho(Ss, None, True)
        xname, cname, DFX, HFX, DFC, fclass = FUN[method]
        acc, mult = GRID[grid]
        ref_atoms = [types.SimpleNamespace(real_vdw_radius=adata[a.symbol]["real_vdw_radius"], ghost=False, origin=a.origin, charge=a.charge)
                     for a in atoms]
        extent = mult * max(a.real_vdw_radius for a in ref_atoms) / 6
        n = int(acc * 9)
        LEB = np.array([3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 35, 41, 47, 53, 59, 65, 71, 77, 83, 89, 95, 101, 107, 113, 119, 125, 131])
        leb = int(LEB[np.abs(LEB - n).argmin()])
        n_radial = int(extent * acc)
        points, weights = dft.build_molecular_grid(extent, n_radial, leb, float(R), ref_atoms)
        bfs = orc.ref_basis_list(aos)
        bfs_on_grid = dft.construct_basis_functions_on_grid(bfs, points, U)
        grads = dft.construct_basis_function_gradients_on_grid(bfs, points, U) if fclass == "GGA" else None
        # core guess
        eps0, C0 = scf.diagonalise_Fock_matrix(Ts_ + Vs, X)
        P0 = scf.construct_density_matrix(C0, nocc, 2)
        E0 = float(np.einsum("mn,mn->", Ts_ + Vs, P0))
        calc = Calc(CONV["extreme"], damping=True)
        calc.DFT_calculation = True
        calc.HFX_prop, calc.DFX_prop, calc.DFC_prop = HFX, DFX, DFC
        calc.X_alpha = 2 / 3
        calc.method = types.SimpleNamespace(name=method)
        calc.functional = types.SimpleNamespace(functional_class=fclass, x_functional=xname, c_functional=cname)
        saved_tab = scf.exchange_correlation_functionals
        scf.exchange_correlation_functionals = {method: calc.functional}
        x_fun = xc.exchange_functionals.get(xname)
        c_fun = xc.correlation_functionals.get(cname)
        # one XC evaluation for the guess density (kernel-level golden)
        V_XC, density, e_X, e_C = scf.calculate_restricted_exchange_correlation_matrix(P0, bfs_on_grid, grads, weights, calc, x_fun, c_fun)
        n_el = float(np.sum(density * weights))
        EX = float(np.sum(e_X * density * weights)) * DFX
        EC = float(np.sum(e_C * density * weights)) * DFC if e_C is not None else 0.0
        n_sph = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
        molecule = types.SimpleNamespace(n_doubly_occ=nocc, partition_ranges=n_sph, atoms=atoms, n_electrons=2 * nocc, n_alpha=nocc, n_beta=nocc)
        table = []
        orig = scf.format_output_line

        def rec(E_total, delta_E, max_DP, RMS_DP, damping_factor, step, commutator, calculation, silent=False):
            table.append([step, E_total, delta_E, RMS_DP, max_DP, commutator, float(damping_factor)])
        scf.format_output_line = rec
        try:
            o = scf.run_self_consistent_field_cycle(molecule, calc, Ints(Ss, Ts_, Vs, Es), mol.nuclear_repulsion(atoms), X, (P0, P0 / 2, P0 / 2, E0),
                                                    (bfs_on_grid, weights, grads, points), True)
        finally:
            scf.format_output_line = orig
            scf.exchange_correlation_functionals = saved_tab
        G = weights.size
        rng = np.random.default_rng(5)
        pick = rng.integers(0, G, 400)
        flat_pts = points.reshape(3, -1)
        d = dict(n_points=G, n_radial=n_radial, lebedev=leb, extent=extent, weights_sum=float(weights.sum()), pick=pick,
                 pts_pick=flat_pts[:, pick], w_pick=weights.reshape(-1)[pick], bfs_pick=bfs_on_grid.reshape(bfs_on_grid.shape[0], -1)[:, pick],
                 dens_pick=density.reshape(-1)[pick], P0=P0, V_XC0=V_XC, n_el0=n_el, EX0=EX, EC0=EC, table=np.array(table), energy=o.energy,
                 components=np.array([o.kinetic_energy, o.nuclear_electron_energy, o.coulomb_energy, o.exchange_energy, o.correlation_energy]),
                 eps=o.epsilons)
        if grads is not None:
            d["grad_pick"] = grads.reshape(3, grads.shape[1], -1)[:, :, pick]
        out[tag] = d
        print("DFT", tag, method, basis, "grid", n_radial, "x", weights.shape[1], "=", G, "pts  n_el", n_el, "E", o.energy, "iters", len(table))
    np.savez_compressed(os.path.join(GOLD, outfile), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


def make_uhf_golden(scf, blocks, ortho):
    """Open-shell systems for the unrestricted path: O2 triplet, NO doublet, OH doublet (hetero), Li atom."""
    out = {}
    for tag, (sym, R, basis, na, nb) in {
        "o2_triplet_sto3g": (["O", "O"], mol.angstrom_to_bohr(1.2075), "STO-3G", 9, 7),
        "o2_triplet_ccpvdz": (["O", "O"], mol.angstrom_to_bohr(1.2075), "cc-pVDZ", 9, 7),
        "no_doublet_631g": (["N", "O"], mol.angstrom_to_bohr(1.1508), "6-31G", 8, 7),
        "oh_doublet_ccpvdz": (["O", "H"], mol.angstrom_to_bohr(0.9697), "cc-pVDZ", 5, 4),
        "li_doublet_631g": (["LI"], None, "6-31G", 2, 1),
    }.items():
        atoms, shells, aos = system(sym, R, basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        U = reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V), eri_to_spherical(U, E)
        d = dict(n_alpha=na, n_beta=nb)
        for damping in (True, False):
            r = run_reference_uhf(scf, ortho, atoms, shells, Ss, Ts_, Vs, Es, na, nb, "extreme", damping)
            sfx = "" if damping else "_nodamp"
            d.update({f"scf_table{sfx}": r["table"], f"scf_energy{sfx}": r["energy"], f"eps_alpha{sfx}": r["epsilons_alpha"],
                      f"eps_beta{sfx}": r["epsilons_beta"], f"components{sfx}": r["components"]})
        d.update(E0=r["E0"], V_NN=r["V_NN"])
        out[tag] = d
        print("UHF", tag, aos.n, "E =", d["scf_energy"], d["scf_energy_nodamp"], "iters", len(d["scf_table"]), len(d["scf_table_nodamp"]))
    np.savez_compressed(os.path.join(GOLD, "uhf_systems.npz"), **{f"{t}__{k}": v for t, d in out.items() for k, v in d.items()})


# Closed-shell systems across H .. Ar and every basis set the reference ships (symbols, bond length in Angstrom or None, basis,
# doubly occupied orbitals -- the charge follows from it).  One reference RHF run each (core guess, EXTREME, dynamic damping).
SWEEP = {
    "h2_augccpvtz": (["H", "H"], 0.74, "aug-cc-pVTZ", 1),
    "heh+_augccpvdz": (["HE", "H"], 0.77, "aug-cc-pVDZ", 1),
    "heh+_ccpvtz": (["HE", "H"], 0.77, "cc-pVTZ", 1),
    "lih_ccpvdz": (["LI", "H"], 1.595, "cc-pVDZ", 2),
    "beh+_6311gss": (["BE", "H"], 1.31, "6-311G**", 2),
    "bh_def2svp": (["B", "H"], 1.232, "def2-SVP", 3),
    "hf_631gs": (["F", "H"], 0.917, "6-31G*", 5),
    "lif_631g": (["LI", "F"], 1.564, "6-31G", 6),
    "co_sto6g": (["C", "O"], 1.128, "STO-6G", 7),
    "n2_321g": (["N", "N"], 1.0977, "3-21G", 7),
    "f2_6311g": (["F", "F"], 1.412, "6-311G", 9),
    "nah_def2svp": (["NA", "H"], 1.887, "def2-SVP", 6),
    "hcl_631gs": (["CL", "H"], 1.275, "6-31G*", 9),
    "alh_631g": (["AL", "H"], 1.648, "6-31G", 7),
    "sio_sto3g": (["SI", "O"], 1.51, "STO-3G", 11),
    "pn_321g": (["P", "N"], 1.491, "3-21G", 11),
    "cl2_631g": (["CL", "CL"], 1.988, "6-31G", 17),
    "nacl_sto6g": (["NA", "CL"], 2.361, "STO-6G", 14),
    "mgh+_631g": (["MG", "H"], 1.65, "6-31G", 6),
    "ne2_augccpvdz": (["NE", "NE"], 3.1, "aug-cc-pVDZ", 10),
    "ar2_def2svp": (["AR", "AR"], 3.76, "def2-SVP", 18),
    "he_ccpv5z": (["HE"], None, "cc-pV5Z", 1),
    "he_augccpvqz": (["HE"], None, "aug-cc-pVQZ", 1),
    "h2_ccpvqz": (["H", "H"], 0.74, "cc-pVQZ", 1),
    "h2_def2qzvp": (["H", "H"], 0.74, "def2-QZVP", 1),
    "h2_def2tzvp": (["H", "H"], 0.74, "def2-TZVP", 1),
    "oh-_def2tzvpp": (["O", "H"], 0.97, "def2-TZVPP", 5),
    "cn-_ccpvdz": (["C", "N"], 1.177, "cc-pVDZ", 7),
    "no+_6311gss": (["N", "O"], 1.063, "6-311G**", 7),
    "be_ccpvtz": (["BE"], None, "cc-pVTZ", 2),
}


def make_sweep_golden(scf, blocks, ortho):
    """tests/golden/sweep_systems.json: per system the reference's RHF energy, iteration count, orbital energies and norms of its
    integral matrices (data only)."""
    import json
    out = {}
    for tag, (sym, R_ang, basis, nocc) in SWEEP.items():
        R = None if R_ang is None else mol.angstrom_to_bohr(R_ang)
        atoms, shells, aos = system(sym, R, basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        U = reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V), eri_to_spherical(U, E)
        r = run_reference_scf(scf, ortho, atoms, shells, Ss, Ts_, Vs, Es, nocc, "extreme", True)
        idx = sample_indices(U.shape[0], 64, 7)
        out[tag] = dict(symbols=sym, R_angstrom=R_ang, basis=basis, n_occ=nocc, n_ao=int(U.shape[0]),
                        energy=float(r["energy"]), V_NN=float(r["V_NN"]), E0=float(r["E0"]), n_iter=int(len(r["table"])),
                        epsilons=[float(x) for x in r["epsilons"]], components=[float(x) for x in r["components"]],
                        S_fro=float(np.linalg.norm(Ss)), T_fro=float(np.linalg.norm(Ts_)), V_fro=float(np.linalg.norm(Vs)),
                        eri_fro=float(np.sqrt(np.sum(Es * Es))), eri_idx=idx.tolist(),
                        eri_val=[float(x) for x in Es[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]])
        print(tag, U.shape[0], "E =", out[tag]["energy"], "iters", out[tag]["n_iter"], flush=True)
    json.dump(out, open(os.path.join(GOLD, "sweep_systems.json"), "w"), indent=0)


FIELD_SYSTEMS = {
    "hf_631g": (["F", "H"], 0.917, "6-31G", 5),
    "lih_sto3g": (["LI", "H"], 1.595, "STO-3G", 2),
    "co_ccpvdz": (["C", "O"], 1.128, "cc-pVDZ", 7),
}


# Open-shell systems for the unrestricted path (symbols, bond length in Angstrom or None, basis, alpha and beta electrons)
UHF_SWEEP = {
    "h_atom_augccpvtz": (["H"], None, "aug-cc-pVTZ", 1, 0),
    "b_atom_631gs": (["B"], None, "6-31G*", 3, 2),
    "c_triplet_ccpvdz": (["C"], None, "cc-pVDZ", 4, 2),
    "n_quartet_def2svp": (["N"], None, "def2-SVP", 5, 2),
    "f_atom_6311g": (["F"], None, "6-311G", 5, 4),
    "na_atom_321g": (["NA"], None, "3-21G", 6, 5),
    "p_quartet_sto6g": (["P"], None, "STO-6G", 9, 6),
    "cl_atom_631g": (["CL"], None, "6-31G", 9, 8),
    "h2+_def2tzvp": (["H", "H"], 1.06, "def2-TZVP", 1, 0),
    "lih+_ccpvdz": (["LI", "H"], 2.2, "cc-pVDZ", 2, 1),
    "beh_6311gss": (["BE", "H"], 1.343, "6-311G**", 3, 2),
    "ch_doublet_ccpvdz": (["C", "H"], 1.12, "cc-pVDZ", 4, 3),
    "nh_triplet_631gs": (["N", "H"], 1.036, "6-31G*", 5, 3),
    "cn_doublet_sto3g": (["C", "N"], 1.172, "STO-3G", 7, 6),
    "o2+_doublet_321g": (["O", "O"], 1.116, "3-21G", 8, 7),
    "b2_triplet_sto3g": (["B", "B"], 1.59, "STO-3G", 6, 4),
}
# members of SWEEP whose RMP2 correlation energy is stored as well (the reference's own AO->MO transformation, tuna_ci.py:204-255)
MP2_SWEEP = ["lih_ccpvdz", "bh_def2svp", "hf_631gs", "lif_631g", "co_sto6g", "n2_321g", "f2_6311g", "hcl_631gs", "alh_631g", "pn_321g",
             "nah_def2svp", "heh+_ccpvtz"]


def make_open_shell_sweep(scf, blocks, ortho):
    """tests/golden/uhf_sweep.json: one reference UHF run per open-shell system (core guess, EXTREME, no damping)."""
    import json
    out = {}
    for tag, (sym, R_ang, basis, na, nb) in UHF_SWEEP.items():
        atoms, shells, aos = system(sym, None if R_ang is None else mol.angstrom_to_bohr(R_ang), basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        U = reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V), eri_to_spherical(U, E)
        try:
            r = run_reference_uhf(scf, ortho, atoms, shells, Ss, Ts_, Vs, Es, na, nb, "extreme", False)
        except RuntimeError as e:                            # the reference's own cycle does not converge without damping: not a fixture
            print("UHF", tag, "skipped:", e, flush=True)
            continue
        out[tag] = dict(symbols=sym, R_angstrom=R_ang, basis=basis, n_alpha=na, n_beta=nb, n_ao=int(U.shape[0]), energy=float(r["energy"]),
                        V_NN=float(r["V_NN"]), E0=float(r["E0"]), n_iter=int(len(r["table"])),
                        eps_alpha=[float(x) for x in r["epsilons_alpha"]], eps_beta=[float(x) for x in r["epsilons_beta"]])
        print("UHF", tag, U.shape[0], "E =", out[tag]["energy"], "iters", out[tag]["n_iter"], flush=True)
    json.dump(out, open(os.path.join(GOLD, "uhf_sweep.json"), "w"), indent=0)


def make_mp2_sweep(scf, blocks, ortho):
    """tests/golden/mp2_sweep.json: RMP2 on the converged reference orbitals of some members of SWEEP (C and eps stored: the
    correlation energy is checked on the SAME orbitals, independent of the SCF's last digits)."""
    import json
    ao_to_mo, doubles_eps = load_reference_ao_to_mo()
    out = {}
    for tag in MP2_SWEEP:
        sym, R_ang, basis, nocc = SWEEP[tag]
        atoms, shells, aos = system(sym, None if R_ang is None else mol.angstrom_to_bohr(R_ang), basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        U = reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V), eri_to_spherical(U, E)
        r = run_reference_scf(scf, ortho, atoms, shells, Ss, Ts_, Vs, Es, nocc, "extreme", True)
        C, eps = r["C"], r["epsilons"]
        ERI_MO = ao_to_mo(Es, C, None, True)
        o, v = slice(0, nocc), slice(nocc, len(eps))
        e_ijab = doubles_eps(eps, eps, o, o, v, v)
        g = ERI_MO.transpose(0, 2, 1, 3)[o, o, v, v]
        E_OS = float(np.einsum("ijab,ijab,ijab->", g, g, e_ijab, optimize=True))
        E_SS = float(np.einsum("ijab,ijab,ijab->", g, g - g.swapaxes(2, 3), e_ijab, optimize=True))
        out[tag] = dict(symbols=sym, R_angstrom=R_ang, basis=basis, n_occ=nocc, E_SCF=float(r["energy"]), E_OS=E_OS, E_SS=E_SS,
                        C=[[float(x) for x in row] for row in C], eps=[float(x) for x in eps])
        print("MP2", tag, len(eps), "E_MP2 =", E_OS + E_SS, flush=True)
    json.dump(out, open(os.path.join(GOLD, "mp2_sweep.json"), "w"), indent=0)


def make_field_golden(scf, blocks, ortho):
    """tests/golden/field_systems.json: the reference's RHF energies in the finite electric fields of its dipole / polarisability /
    hyperpolarisability drivers (tuna_energy.py:315-650: field term F = sum_i E_i D_i, kernel:660-677; core guess, EXTREME, dynamic
    damping) and the derivatives its own formulas (tuna_util.py:581-680, evaluated from the source text) make of them.  Data only."""
    import ast
    import json
    util_src = open(os.path.join(REF, "TUNA", "tuna_util.py")).read()
    lines, _ = _parseable_lines(os.path.join(REF, "TUNA", "tuna_util.py"))
    tree = ast.parse("\n".join(lines))
    ns = {}
    steps = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in ("calculate_first_derivative", "calculate_second_derivative", "calculate_third_derivative"):
            node.returns = None
            for a in node.args.args:
                a.annotation = None
            exec(compile(ast.Module([node], []), "tuna_util.py", "exec"), ns)
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and \
                node.targets[0].id in ("FIRST_ELEC_DERIVATIVE_STEP", "SECOND_ELEC_DERIVATIVE_STEP", "THIRD_ELEC_DERIVATIVE_STEP"):
            steps[node.targets[0].id] = float(ast.literal_eval(node.value))
    h1, h2, h3 = steps["FIRST_ELEC_DERIVATIVE_STEP"], steps["SECOND_ELEC_DERIVATIVE_STEP"], steps["THIRD_ELEC_DERIVATIVE_STEP"]
    out = {}
    for tag, (sym, R_ang, basis, nocc) in FIELD_SYSTEMS.items():
        atoms, shells, aos = system(sym, mol.angstrom_to_bohr(R_ang), basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        U = reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V), eri_to_spherical(U, E)
        Ds = np.array([to_spherical(U, D[k]) for k in range(3)])

        def energy(field):
            F = np.einsum("i,ijk->jk", np.asarray(field, dtype=float), Ds, optimize=True)      # kernel:675
            return float(run_reference_scf(scf, ortho, atoms, shells, Ss, Ts_, Vs, Es, nocc, "extreme", True, F_fld=F)["energy"])
        x, z = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
        E0 = energy(0 * z)
        dip = {"+z": energy(h1 * z), "-z": energy(-h1 * z)}
        pol = {k: energy(h2 * f) for k, f in {"+2z": 2 * z, "+z": z, "-z": -z, "-2z": -2 * z, "+2x": 2 * x, "+x": x, "-x": -x, "-2x": -2 * x}.items()}
        hyp = {k: energy(h3 * f) for k, f in {"+3z": 3 * z, "+2z": 2 * z, "+z": z, "-z": -z, "-2z": -2 * z, "-3z": -3 * z, "-4z": -4 * z,
                                                "+4z": 4 * z, "+x+z": x + z, "-x+z": -x + z, "+x-z": x - z, "-x-z": -x - z}.items()}
        d1, d2, d3 = ns["calculate_first_derivative"], ns["calculate_second_derivative"], ns["calculate_third_derivative"]
        out[tag] = dict(symbols=sym, R_angstrom=R_ang, basis=basis, n_occ=nocc, n_ao=int(U.shape[0]), dipole_origin_z=float(com_z(atoms)),
                        steps=[h1, h2, h3], energy=E0, dipole_energies=dip, polarisability_energies=pol, hyperpolarisability_energies=hyp,
                        electronic_dipole=-1 * d1(dip["-z"], dip["+z"], h1),
                        polarisability_parallel=-1 * d2(pol["-2z"], pol["-z"], E0, pol["+z"], pol["+2z"], h2),
                        polarisability_perpendicular=-1 * d2(pol["-2x"], pol["-x"], E0, pol["+x"], pol["+2x"], h2),
                        hyperpolarisability_parallel=-1 * d3(hyp["-4z"], hyp["-3z"], hyp["-2z"], hyp["-z"], hyp["+z"], hyp["+2z"], hyp["+3z"],
                                                             hyp["+4z"], h3),
                        hyperpolarisability_perpendicular=-(hyp["-x+z"] - 2 * hyp["+z"] + hyp["+x+z"] - hyp["-x-z"] + 2 * hyp["-z"]
                                                            - hyp["+x-z"]) / (2 * h3 ** 3))        # energy:541
        print(tag, U.shape[0], "E0 =", E0, "alpha", out[tag]["polarisability_parallel"], out[tag]["polarisability_perpendicular"],
              "beta", out[tag]["hyperpolarisability_parallel"], out[tag]["hyperpolarisability_perpendicular"], flush=True)
    json.dump(out, open(os.path.join(GOLD, "field_systems.json"), "w"), indent=0)



KEYWORD_CASES = {
    # tag: (keywords of the input line, fields of the reference Calculation they set)
    "base": ("", {}),
    "ez": ("EZ 0.01", {"field": [0.0, 0.0, 0.01]}),
    "ex_ez": ("EX 0.005 EZ -0.002", {"field": [0.005, 0.0, -0.002]}),
    "egz": ("EGZ 0.01", {"gradient": [0.0, 0.0, 0.01]}),
    "egx_egy": ("EGX 0.004 EGY 0.002", {"gradient": [0.004, 0.002, 0.0]}),
    "conv": ("ECONV 1e-4 RMSDP 1e-3 MAXDP 1e-3 DIISERR 1e-2", {"conv": {"delta_E": 1e-4, "RMS_DP": 1e-3, "max_DP": 1e-3, "commutator": 1e-2}}),
    "diis10": ("EXTREME DIIS 10 NODAMP", {"max_diis": 10, "conv_name": "extreme", "damping": False}),
    "diis12_damp": ("EXTREME DIIS 12", {"max_diis": 12, "conv_name": "extreme"}),
}


def make_keyword_golden(scf, blocks, ortho):
    """tests/golden/keyword_runs.json: the reference's RHF cycle (core guess) under the SCF keywords of tuna_calc.py:153-165,187-190
    (EX/EY/EZ, EGX/EGY/EGZ through kernel:660-707 executed from the source text; ECONV/RMSDP/MAXDP/DIISERR through calc:491-494;
    DIIS n with n > 8) for two small systems: energies and iteration tables.  Data only."""
    import ast
    import json
    lines, _ = _parseable_lines(os.path.join(REF, "TUNA", "tuna_kernel.py"))
    tree = ast.parse("\n".join(lines))
    ns = {"np": np}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in ("apply_electric_field", "apply_electric_field_gradient"):
            node.returns = None
            for a in node.args.args:
                a.annotation = None
            exec(compile(ast.Module([node], []), "tuna_kernel.py", "exec"), ns)
    out = {}
    for sysname, (sym, R_ang, basis, nocc) in {"hf_631g": (["F", "H"], 0.917, "6-31G", 5), "co_ccpvdz": (["C", "O"], 1.128, "cc-pVDZ", 7)}.items():
        atoms, shells, aos = system(sym, mol.angstrom_to_bohr(R_ang), basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        # dipole / quadrupole integrals about the centre of mass, as the input line has them (kernel:312; the masses are the reference's table)
        from tuna_amd import guess as guess_mod
        com = guess_mod.centre_of_mass(atoms)
        _, _, _, D, Q = orc.ref_one_electron(aos, [a.origin for a in atoms], [float(a.charge) for a in atoms], [0.0, 0.0, com])
        U = reference_U(shells, blocks)
        Ss, Ts_, Vs, Es = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V), eri_to_spherical(U, E)
        Ds = np.array([to_spherical(U, D[k]) for k in range(3)])
        Qs = np.array([to_spherical(U, Q[k]) for k in range(len(Q))])
        X, smallest, S_inv = ortho(Ss, None, True)
        eps0, C0 = scf.diagonalise_Fock_matrix(Ts_ + Vs, X)
        P0 = scf.construct_density_matrix(C0, nocc, 2)
        E0 = float(np.einsum("mn,mn->", Ts_ + Vs, P0))
        n_sph = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
        molecule = types.SimpleNamespace(n_doubly_occ=nocc, partition_ranges=n_sph, atoms=atoms, n_electrons=2 * nocc, n_alpha=nocc, n_beta=nocc)
        cases = {}
        for tag, (kw, f) in KEYWORD_CASES.items():
            conv = dict(CONV[f.get("conv_name", "medium")])
            conv.update(f.get("conv", {}))                                   # calc:491-494
            calc = Calc(conv, damping=f.get("damping", True))
            calc.max_DIIS_matrices = f.get("max_diis", 6)
            ints = Ints(Ss, Ts_, Vs, Es)
            if "field" in f:
                ints.F = ns["apply_electric_field"](Ds, np.array(f["field"]))                  # energy:915
            if "gradient" in f:
                ints.G = ns["apply_electric_field_gradient"](Qs, np.array(f["gradient"]))      # energy:919
            table = []
            orig = scf.format_output_line

            def rec(E_total, delta_E, max_DP, RMS_DP, damping_factor, step, commutator, calculation, silent=False):
                table.append([step, E_total, delta_E, RMS_DP, max_DP, commutator, float(damping_factor)])
            scf.format_output_line = rec
            try:
                o = scf.run_self_consistent_field_cycle(molecule, calc, ints, mol.nuclear_repulsion(atoms), X, (P0, P0 / 2, P0 / 2, E0),
                                                        (None, None, None, None), True)
            finally:
                scf.format_output_line = orig
            cases[tag] = dict(keywords=kw, energy=float(o.energy), iterations=len(table), table=[[float(x) for x in row] for row in table],
                              field_energy=float(o.electric_field_energy), field_gradient_energy=float(o.electric_field_gradient_energy))
            print(sysname, tag, kw, "E =", o.energy, "iterations", len(table), flush=True)
        out[sysname] = dict(symbols=sym, R_angstrom=R_ang, basis=basis, n_occ=nocc, smallest_overlap_eigenvalue=float(smallest), dipole_origin_z=float(com), cases=cases)
    json.dump(out, open(os.path.join(GOLD, "keyword_runs.json"), "w"), indent=0)


def random_basis_system():
    """The C-F pair with random exponents (s, p, d, f and g shells) of tests/test_oracle.py's direct check."""
    rng = np.random.default_rng(7)
    basis = {6: [("S", [(float(rng.uniform(0.3, 8)), 0.4), (float(rng.uniform(0.1, 0.3)), 0.7)]),
                 ("P", [(float(rng.uniform(0.2, 3)), 1.0)]), ("F", [(float(rng.uniform(0.3, 2)), 1.0)])],
             9: [("S", [(float(rng.uniform(0.3, 5)), 1.0)]), ("D", [(float(rng.uniform(0.2, 2)), 0.5), (0.31, 0.6)]),
                 ("G", [(0.9, 1.0)])]}
    return system(["C", "F"], 2.3, basis)


def unique_eri_index(n):
    """Flat position of every (i, j, k, l) among the 8-fold unique values: pair (ij) = i(i+1)/2 + j for i >= j, quartet
    (ij)((ij)+1)/2 + (kl) for (ij) >= (kl) -- the order of the reference's own loop (pyx:1300-1338), which writes each
    value it computes to all eight images, so these values determine its tensor exactly."""
    i, j, k, l = np.indices((n,) * 4)
    ij = np.maximum(i, j) * (np.maximum(i, j) + 1) // 2 + np.minimum(i, j)
    kl = np.maximum(k, l) * (np.maximum(k, l) + 1) // 2 + np.minimum(k, l)
    return np.maximum(ij, kl) * (np.maximum(ij, kl) + 1) // 2 + np.minimum(ij, kl)


def make_random_basis_golden():
    """The compiled reference engine on random_basis_system(): one-electron matrices in full, the ERI tensor as its 8-fold unique
    values (unique_eri_index).  Data only."""
    atoms, shells, aos = random_basis_system()
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    S, T, V, D, Q = orc.ref_one_electron(aos, xyz, chg, [0, 0, 1.0])
    E = orc.ref_eri(aos)
    npair = aos.n * (aos.n + 1) // 2
    eri_unique = np.zeros(npair * (npair + 1) // 2)
    eri_unique[unique_eri_index(aos.n).ravel()] = E.ravel()
    np.savez_compressed(os.path.join(GOLD, "random_basis.npz"), S=S, T=T, V=V, D=D, Q=Q, eri_unique=eri_unique,
                        exps=aos.exps, coefs=aos.coefs, lmn=aos.lmn, origin=aos.origin, prim_off=aos.prim_off)
    print("random_basis", aos.n, len(eri_unique))


def run_reference_scf(scf, ortho, atoms, shells, S, T, V, ERI, n_occ, conv="extreme", damping=True, F_fld=None):
    """Core-Hamiltonian guess (tuna_guess.py calculate_core_guess: diagonalise H_core, fill n_occ) + reference loop."""
    X, smallest, S_inv = ortho(S, None, True)
    eps0, C0 = scf.diagonalise_Fock_matrix(T + V, X)
    P0 = scf.construct_density_matrix(C0, n_occ, 2)
    E0 = float(np.einsum("mn,mn->", T + V, P0))
    n_sph = [sum(s.n_sph for s in shells if s.atom == a) for a in range(len(atoms))]
    molecule = types.SimpleNamespace(n_doubly_occ=n_occ, partition_ranges=n_sph, atoms=atoms,
                                     n_electrons=2 * n_occ, n_alpha=n_occ, n_beta=n_occ)
    table = []
    orig = scf.format_output_line

    def rec(E_total, delta_E, max_DP, RMS_DP, damping_factor, step, commutator, calculation, silent=False):
        table.append([step, E_total, delta_E, RMS_DP, max_DP, commutator, float(damping_factor)])
    scf.format_output_line = rec
    try:
        V_NN = mol.nuclear_repulsion(atoms)
        ints = Ints(S, T, V, ERI)
        if F_fld is not None:
            ints.F = F_fld                                   # energy:915 (set after the guess: the core guess does not see the field)
        out = scf.run_self_consistent_field_cycle(molecule, Calc(CONV[conv], damping=damping), ints, V_NN, X,
                                                  (P0, P0 / 2, P0 / 2, E0), (None, None, None, None), True)
    finally:
        scf.format_output_line = orig
    return dict(table=np.array(table), energy=out.energy, epsilons=out.epsilons, C=out.molecular_orbitals, P=out.P, X=X, P0=P0, E0=E0,
                V_NN=V_NN, components=np.array([out.kinetic_energy, out.nuclear_electron_energy, out.coulomb_energy,
                                                out.exchange_energy]), smallest_S=smallest)


# --------------------------------------------------------------------------------------------

def main():
    os.makedirs(GOLD, exist_ok=True)
    assert orc.ref_engine() is not None, "run oracle/build_ref.sh first"
    if "--random-basis-only" in sys.argv:
        make_random_basis_golden()
        return
    scf = load_reference_scf()
    blocks, ortho = load_reference_kernel_bits()
    if "--uhf-only" in sys.argv:
        make_uhf_golden(scf, blocks, ortho)
        return
    if "--dft-only" in sys.argv:
        make_dft_golden(scf, blocks, ortho)
        return
    if "--dft-sweep-only" in sys.argv:
        make_dft_golden(scf, blocks, ortho, {t: (sym, mol.angstrom_to_bohr(R), basis, nocc, m, g)
                                             for t, (sym, R, basis, nocc, m, g) in DFT_FUNCTIONAL_SWEEP.items()}, "dft_functionals.npz")
        return
    if "--sad-only" in sys.argv:
        make_sad_golden(scf, blocks, ortho)
        return
    if "--mp2-only" in sys.argv:
        make_mp2_golden(scf, blocks, ortho)
        return
    if "--uhf-sweep-only" in sys.argv:
        make_open_shell_sweep(scf, blocks, ortho)
        return
    if "--mp2-sweep-only" in sys.argv:
        make_mp2_sweep(scf, blocks, ortho)
        return
    if "--field-only" in sys.argv:
        make_field_golden(scf, blocks, ortho)
        return
    if "--keywords-only" in sys.argv:
        make_keyword_golden(scf, blocks, ortho)
        return
    if "--sweep-only" in sys.argv:
        make_sweep_golden(scf, blocks, ortho)
        return
    np.savez(os.path.join(GOLD, "sph_blocks.npz"), **{f"L{L}": b for L, b in blocks.items()})

    # Boys function samples straight from the routine the reference calls (pyx:1505)
    from scipy.special import hyp1f1
    Ts = np.concatenate([[0.0, 1e-12, 1e-8, 1e-4], np.logspace(-3, 4, 141), np.linspace(30, 40, 41),
                         np.arange(0, 36, 1 / 16.0) + 1 / 32.0])
    ms = np.arange(0, 25)
    F = np.array([[hyp1f1(m + 0.5, m + 1.5, -T) / (2.0 * m + 1.0) for T in Ts] for m in ms])
    np.savez(os.path.join(GOLD, "boys.npz"), T=Ts, m=ms, F=F)

    R_H2 = mol.angstrom_to_bohr(0.74)
    R_N2 = mol.angstrom_to_bohr(1.0977)
    R_CO = mol.angstrom_to_bohr(1.128)
    R_AR2 = mol.angstrom_to_bohr(3.76)

    # ---- small systems: everything stored in full -----------------------------------------
    small = {}
    for tag, (sym, R, basis, nocc) in {
        "h2_sto3g_1p4": (["H", "H"], 1.4, "STO-3G", 1),
        "h2_sto3g": (["H", "H"], R_H2, "STO-3G", 1),
        "n2_sto3g": (["N", "N"], R_N2, "STO-3G", 7),
        "he_631g": (["HE"], None, "6-31G", 1),
    }.items():
        atoms, shells, aos = system(sym, R, basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        U = reference_U(shells, blocks)
        bl = orc.ref_basis_list(aos)
        d = dict(S=S, T=T, V=V, D=D, Q=Q, ERI=E, U=U,
                 norm=np.concatenate([np.asarray(b.norm) for b in bl]),
                 coefs=np.concatenate([np.asarray(b.coefs) for b in bl]),
                 lmn=aos.lmn, origin=aos.origin, prim_off=aos.prim_off)
        Ss, Ts_, Vs, Es = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V), eri_to_spherical(U, E)
        for damping in (True, False):
            r = run_reference_scf(scf, ortho, atoms, shells, Ss, Ts_, Vs, Es, nocc, "extreme", damping)
            sfx = "" if damping else "_nodamp"
            d.update({f"scf_table{sfx}": r["table"], f"scf_energy{sfx}": r["energy"], f"scf_eps{sfx}": r["epsilons"],
                      f"scf_P{sfx}": r["P"], f"scf_components{sfx}": r["components"]})
        d.update(X=r["X"], P0=r["P0"], E0=r["E0"], V_NN=r["V_NN"])
        small[tag] = d
        print(tag, aos.n, "E =", d["scf_energy"], "iters", len(d["scf_table"]), len(d["scf_table_nodamp"]))
    np.savez_compressed(os.path.join(GOLD, "small_systems.npz"),
                        **{f"{t}__{k}": v for t, d in small.items() for k, v in d.items()})

    # ---- BASELINE configs: samples + matrices + reference SCF trajectories ------------------
    rngP = np.random.default_rng(0)
    for tag, (sym, R, basis, nocc, nsample) in {
        "c2_n2_ccpvtz": (["N", "N"], R_N2, "cc-pVTZ", 7, 20000),
        "c4_co_def2tzvp": (["C", "O"], R_CO, "def2-TZVP", 7, 20000),
        "n2_ccpvdz": (["N", "N"], R_N2, "cc-pVDZ", 7, 20000),
        "c3_ar2_ccpvqz": (["AR", "AR"], R_AR2, "cc-pVQZ", 18, 20000),
    }.items():
        atoms, shells, aos = system(sym, R, basis)
        S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
        U = reference_U(shells, blocks)
        bl = orc.ref_basis_list(aos)
        idx = sample_indices(aos.n, nsample, 1)
        d = dict(S=S, T=T, V=V, D=D, Q=Q, U=U, lmn=aos.lmn, prim_off=aos.prim_off,
                 norm=np.concatenate([np.asarray(b.norm) for b in bl]),
                 coefs=np.concatenate([np.asarray(b.coefs) for b in bl]),
                 eri_idx=idx, eri_val=E[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]],
                 eri_fro=np.sqrt(np.sum(E * E)), eri_sum=np.sum(E), eri_nonzero_frac=np.mean(E != 0.0))
        Es = eri_to_spherical(U, E)
        del E
        ns = U.shape[0]
        idxs = sample_indices(ns, nsample, 2)
        d.update(eri_sph_idx=idxs, eri_sph_val=Es[idxs[:, 0], idxs[:, 1], idxs[:, 2], idxs[:, 3]],
                 eri_sph_fro=np.sqrt(np.sum(Es * Es)))
        Ss, Ts_, Vs = to_spherical(U, S), to_spherical(U, T), to_spherical(U, V)
        A = rngP.standard_normal((ns, ns))
        P = A + A.T
        P *= 2 * nocc / np.trace(P @ Ss)
        d.update(P_rand=P, J_rand=scf.calculate_coulomb_matrix(P, Es), K_rand=scf.calculate_exchange_matrix(P, Es))
        for damping in (True, False):
            r = run_reference_scf(scf, ortho, atoms, shells, Ss, Ts_, Vs, Es, nocc, "extreme", damping)
            sfx = "" if damping else "_nodamp"
            d.update({f"scf_table{sfx}": r["table"], f"scf_energy{sfx}": r["energy"], f"scf_eps{sfx}": r["epsilons"],
                      f"scf_components{sfx}": r["components"]})
        d.update(V_NN=r["V_NN"], E0=r["E0"], smallest_S=r["smallest_S"])
        del Es
        np.savez_compressed(os.path.join(GOLD, f"{tag}.npz"), **d)
        print(tag, aos.n, ns, "E =", d["scf_energy"], d["scf_energy_nodamp"], "iters", len(d["scf_table"]),
              len(d["scf_table_nodamp"]))

    # ---- high angular momentum coverage (s..h shells, single primitives) ----------------------
    hb = {7: [("S", [(1.3, 1.0)]), ("P", [(0.9, 1.0)]), ("D", [(1.1, 1.0)]), ("F", [(0.8, 1.0)]), ("G", [(1.0, 1.0)]),
              ("H", [(0.7, 1.0)])],
          8: [("S", [(2.0, 0.6), (0.5, 0.5)]), ("D", [(0.9, 0.7), (0.4, 0.4)]), ("H", [(1.2, 1.0)])]}
    atoms, shells, aos = system(["N", "O"], 2.1, hb)
    S, T, V, D, Q, E = one_e_and_eri(atoms, aos)
    U = reference_U(shells, blocks)
    idx = sample_indices(aos.n, 40000, 3)
    Es = eri_to_spherical(U, E)
    idxs = sample_indices(U.shape[0], 40000, 4)
    np.savez_compressed(os.path.join(GOLD, "high_l.npz"), S=S, T=T, V=V, D=D, Q=Q, U=U, lmn=aos.lmn,
                        eri_idx=idx, eri_val=E[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]],
                        eri_fro=np.sqrt(np.sum(E * E)), eri_sph_idx=idxs,
                        eri_sph_val=Es[idxs[:, 0], idxs[:, 1], idxs[:, 2], idxs[:, 3]],
                        eri_sph_fro=np.sqrt(np.sum(Es * Es)))
    print("high_l", aos.n, U.shape[0])
    make_uhf_golden(scf, blocks, ortho)
    make_mp2_golden(scf, blocks, ortho)
    make_sad_golden(scf, blocks, ortho)
    make_dft_golden(scf, blocks, ortho)
    make_random_basis_golden()


if __name__ == "__main__":
    main()
