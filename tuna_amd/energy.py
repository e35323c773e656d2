"""Energy driver: the hot-path subset of tuna_energy.calculate_energy (energy:875-964) and tuna.py's input line.

    from tuna_amd.energy import run
    out = run("SPE : N N 1.0977 : HF CC-PVTZ : EXTREME NODAMP")

Input line format `TYPE : A B R : METHOD BASIS : KEYWORDS` (tuna.py:87-99).  Supported here: TYPE = SPE, METHOD = HF
(restricted) or UHF / any multiplicity via ML (unrestricted), a functional of tuna_amd.dft.FUNCTIONALS (restricted Kohn-Sham; unrestricted
with ML n >= 2, or with a U prefix such as UB3LYP), the basis sets shipped in tuna_amd/data, and the SCF keywords of SURVEY.md section 5
(LOOSE/MEDIUM/TIGHT/EXTREME, MAXITER n, DIIS [n]/NODIIS, DAMP x/NODAMP/MAXDAMP x, SLOWCONV/VERYSLOWCONV, HFX x,
CARTHARM, DECONTRACT, COREGUESS/SADGUESS, CH n, ML n).  After the SCF: MP2 / MP3 and their SCS forms, MP4(SDQ) / MP4(DQ) (also written
MP4[SDQ] / MP4[DQ]; full MP4 with triples through Calculation.mp4 = "SDTQ", not on the input line), and the coupled-cluster doubles
methods LCCD and CCD on a closed-shell restricted reference (AMPCONV x, CORRMAXITER n, CORRDAMP [x]; DIIS n / NODIIS act on their
iterations too), and the vertical excitation spectrum of a closed-shell restricted reference: CIS, TDHF / RPA, TD on an HF line, or TD on
the line of a local-density functional (tuna_amd.dft.TD_AVAILABLE: TD-DFT with the exchange-correlation kernel on the device)
(TDA, NSTATES n, ROOT n / STATE n, NOSINGLETS, NOTRIPLETS, EXTHRESH x; (D) or [D] adds CIS(D) to the ROOT state), and STAB, the stability analysis of a Hartree-Fock SCF (RHF or UHF) in front
of any post-SCF stage.  Through calculate_energy, a Calculation with reference "UHF" and excited_state set runs the spin-conserving CIS /
TDHF of the open shell -- with a functional of tuna_amd.dft.TD_AVAILABLE, unrestricted TD-DFT / TDA (run_unrestricted_tddft) -- and a
Calculation with stability_analysis set and such a functional the stability analysis of the Kohn-Sham solution, restricted or
unrestricted (run_kohn_sham_stability); the input lines of both stay refused.  Everything numerical runs on the GPU through the C ABI.  The initial
guess is the reference's default for single points, the superposition of atomic densities (tuna_amd/guess.py).
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from . import molecule as mol
from ._lib import TunaError
from .engine import SCF_CONVERGENCE, Engine
from .scf import BIG_SPACER, SPACER, DeviceERI, Integrals, construct_density_matrix, run_self_consistent_field_cycle


@dataclass
class Calculation:
    """The fields of the reference's Calculation (tuna_calc.py:532-596) that the hot path reads."""
    calculation_type: str = "SPE"
    method: str = "HF"
    basis: str = "STO-3G"
    reference: str = "RHF"
    charge: int = 0
    SCF_conv: dict = field(default_factory=lambda: SCF_CONVERGENCE["medium"])
    max_iter: int = 100                 # MAXITER, calc:158
    DIIS: bool = True                   # calc:198
    max_DIIS_matrices: int = 6
    damping: bool = True                # calc:199
    damping_factor: float | None = None
    max_damping: float = 0.7            # calc:159
    HFX_prop: float = 1.0               # calc:207
    cartesian_harmonics: bool = False   # CARTHARM, calc:91
    decontract: bool = False            # DECONTRACT, calc:90
    core_guess: bool = False            # COREGUESS, calc:95; default is the superposition of atomic densities
    DFT_calculation: bool = False
    multiplicity: int = 1               # ML, calc:151
    functional: str | None = None       # Kohn-Sham functional name (tuna_amd.dft.FUNCTIONALS) or None for Hartree-Fock
    grid_conv: str = "medium"           # LOOSEGRID/MEDIUMGRID/TIGHTGRID..., util:129-137
    X_alpha: float = 2 / 3              # XA, calc:156
    dipole: bool = False                # DIPOLE, calc:137: finite-field electric properties (tuna_amd/properties.py)
    polarisability: bool = False        # POLAR, calc:139
    hyperpolarisability: bool = False   # HYPER, calc:140
    electric_field: tuple = (0.0, 0.0, 0.0)            # EX, EY, EZ, calc:160-162, 431
    electric_field_gradient: tuple = (0.0, 0.0, 0.0)   # EGX, EGY, EGZ, calc:163-165, 432
    S_eigenvalue_threshold: float = 1e-7               # STHRESH, calc:157
    number_of_threads: int = 4                         # THREADS, calc:153 (host threads of the reference's OpenMP loops: no meaning here)
    spin_component_scaling: bool = False               # SCS-MP2 / USCS-MP2 (tuna_mp.py:872, :1042)
    same_spin_scaling: float = 1 / 3                   # SSS, calc:208
    opposite_spin_scaling: float = 6 / 5               # OSS, calc:209
    mp3: bool = False                                  # MP3 / SCS-MP3 after the MP2 step (tuna_mp.py:1814-1828)
    MP3_scaling: float = 1 / 4                         # MP3S / MP3SCALING / MP3SCAL, calc:183 (applied by SCS-MP3 only)
    mp4: str | None = None                             # "SDQ" or "DQ": MP4(SDQ) / MP4(DQ) after MP2 and MP3 (tuna_mp.py:1552-1685);
                                                       # "SDTQ": full MP4 with the triples (not on the input line yet)
    coupled_cluster: str | None = None                 # "LCCD" or "CCD" after the SCF (tuna_cc.py:830-864, :915-960), or "LCCSD",
                                                       # "QCISD", "CCSD" (:1020-1063, :1503-1557, :1638-1718; not on the input line yet)
    triples: bool = False                              # the perturbative triples after CCSD or QCISD: CCSD(T), QCISD(T) (tuna_cc.py:2688-2758)
    amp_conv: float = 1e-8                             # AMPCONV, calc:184
    correlated_max_iter: int = 100                     # CORRMAXITER, calc:191
    correlated_damping_parameter: float = 0.0          # CORRDAMP [x], calc:201 (without a number: the default, no damping)
    excited_state: str | None = None                   # the printed name of an excited-state run: "CIS", "TDHF", "RPA" or "TD-HF"
    time_dependent: bool = False                       # TD, calc:114
    tamm_dancoff_approximation: bool = False           # TDA, calc:113 (always on for CIS, tuna_ci.py:1314)
    calculate_no_singlets: bool = False                # NOSINGLETS, calc:120
    calculate_no_triplets: bool = False                # NOTRIPLETS, calc:119
    root: int = 1                                      # ROOT / STATE, calc:167
    n_states: int = 10                                 # NSTATES, calc:169
    excited_state_contribution_threshold: float = 1.0  # EXTHRESH (per cent), calc:168
    do_perturbative_doubles: bool = False              # (D) / [D], calc:121: CIS(D) of the ROOT state after the spectrum (tuna_ci.py:2293-2295)
    relaxed_density: bool = False                      # RELAXED: the Z-vector relaxed MP2 density (tuna_mp.py:908, :939-945)
    unrelaxed_density: bool = False                    # UNRELAXED: the unrelaxed MP2 density, the reference's default
    natural_orbitals: bool = False                     # NATORBS: natural orbitals of the MP2 density (tuna_mp.py:971-973)
    stability_analysis: bool = False                   # STAB, calc:118: the lowest orbital-Hessian eigenvalues after the SCF (kernel:1146)
    freeze_core: bool = False                          # read by the unrestricted excited states and STAB only (tuna_ci.py:545, :650): the
                                                       # core orbitals of FROZEN_CORE_ORBITALS stay out of the occupied window of either spin


@dataclass
class Molecule:
    atoms: list
    shells: list
    aos: mol.AOList
    n_electrons: int
    n_doubly_occ: int
    n_alpha: int
    n_beta: int
    partition_ranges: list
    n_basis: int
    n_cartesian_basis: int


def parse_input(input_line: str):
    """tuna.py:59-161 -> (calculation_type, method, basis, atomic_symbols, R_bohr | None, params)."""
    try:
        sections = input_line.upper().strip().split(":")
        calculation_type = sections[0].strip()
        geometry = [g for g in sections[1].strip().split(" ") if g.strip()]
        method, basis = sections[2].strip().split()
        params = sections[3].strip().split() if len(sections) == 4 else []
    except Exception:
        raise TunaError("Input line formatted incorrectly! Read the manual for help.")
    symbols = geometry[:2] if len(geometry) >= 3 else geometry[:1]
    try:
        R = [float(x) for x in geometry[len(symbols):]]
    except ValueError:
        raise TunaError("Could not parse bond length!")
    if len(symbols) == 2 and len(R) != 1:
        raise TunaError("Two atoms requested without a bond length!")
    if R and R[0] < 0.01:
        raise TunaError(f"Bond length ({R[0]} angstroms) is too small! Minimum bond length is 0.01 angstroms.")
    return calculation_type, method, basis, symbols, (mol.angstrom_to_bohr(R[0]) if R else None), params


def interpret_keywords(params, calc: Calculation) -> Calculation:
    """The SCF subset of tuna_calc.py:83-217, 357-521."""
    it = iter(range(len(params)))
    custom = {}
    for k in it:
        p = params[k]

        def value():
            try:
                next(it)
                return params[k + 1]
            except (StopIteration, IndexError):
                raise TunaError(f"Keyword {p} needs a value")
        if p in ("LOOSE", "MEDIUM", "TIGHT", "EXTREME"):
            calc.SCF_conv = SCF_CONVERGENCE[p.lower()]
        elif p == "MAXITER":
            calc.max_iter = int(value())
        elif p == "NODIIS":
            calc.DIIS = False
        elif p == "DIIS":
            if k + 1 < len(params) and params[k + 1].isdigit():
                calc.max_DIIS_matrices = int(value())
        elif p == "NODAMP":
            calc.damping = False
        elif p == "DAMP":
            calc.damping, calc.damping_factor = True, float(value())
        elif p == "SLOWCONV":
            calc.damping, calc.damping_factor = True, 0.5
        elif p == "VERYSLOWCONV":
            calc.damping, calc.damping_factor = True, 0.85
        elif p == "MAXDAMP":
            calc.max_damping = float(value())
        elif p == "HFX":
            calc.HFX_prop = float(value())
        elif p == "CARTHARM":
            calc.cartesian_harmonics = True
        elif p == "DECONTRACT":
            calc.decontract = True
        elif p in ("CH", "CHARGE"):
            calc.charge = int(value())
        elif p in ("ML", "MULTIPLICITY"):
            calc.multiplicity = int(value())
        elif p in ("LOOSEGRID", "MEDIUMGRID", "TIGHTGRID", "EXTREMEGRID"):
            calc.grid_conv = p[:-4].lower()
        elif p == "XA":
            calc.X_alpha = float(value())
        elif p == "COREGUESS":
            calc.core_guess = True
        elif p == "DIPOLE":
            calc.dipole = True
        elif p in ("POLAR", "POLARISABILITY", "POLARIZABILITY"):
            calc.polarisability = True
        elif p in ("HYPER", "HYPERPOLARISABILITY", "HYPERPOLARIZABILITY"):
            calc.hyperpolarisability = True
        elif p == "THREADS":
            calc.number_of_threads = int(value())           # accepted and ignored: the integrals run on the GPU
        elif p == "STHRESH":
            calc.S_eigenvalue_threshold = float(value())
        elif p == "SSS":                                     # accepted on plain MP2 as in the reference, where it changes nothing
            calc.same_spin_scaling = float(value())
        elif p == "OSS":
            calc.opposite_spin_scaling = float(value())
        elif p in ("MP3S", "MP3SCALING", "MP3SCAL"):
            calc.MP3_scaling = float(value())
        elif p == "AMPCONV":
            calc.amp_conv = float(value())
        elif p == "CORRMAXITER":
            calc.correlated_max_iter = int(value())
        elif p == "CORRDAMP":                                # a boolean with an optional value (calc:201, as DIIS above)
            calc.correlated_damping_parameter = 0.0
            if k + 1 < len(params):
                try:
                    x = float(params[k + 1])
                except ValueError:
                    x = None
                if x is not None:
                    calc.correlated_damping_parameter = x
                    next(it)
        elif p == "TD":
            calc.time_dependent = True
        elif p == "TDA":
            calc.tamm_dancoff_approximation = True
        elif p == "NOSINGLETS":
            calc.calculate_no_singlets = True
        elif p == "NOTRIPLETS":
            calc.calculate_no_triplets = True
        elif p in ("ROOT", "STATE"):
            calc.root = int(value())
        elif p == "NSTATES":
            calc.n_states = int(value())
        elif p == "EXTHRESH":
            calc.excited_state_contribution_threshold = float(value())
        elif p in ("(D)", "[D]"):
            calc.do_perturbative_doubles = True
        elif p == "RELAXED":
            calc.relaxed_density = True
        elif p == "UNRELAXED":
            calc.unrelaxed_density = True
        elif p == "NATORBS":
            calc.natural_orbitals = True
        elif p == "STAB":
            calc.stability_analysis = True
        elif p in ("EX", "EY", "EZ"):
            f = list(calc.electric_field)
            f["XYZ".index(p[1])] = float(value())
            calc.electric_field = tuple(f)
        elif p in ("EGX", "EGY", "EGZ"):
            f = list(calc.electric_field_gradient)
            f["XYZ".index(p[2])] = float(value())
            calc.electric_field_gradient = tuple(f)
        elif p in ("ECONV", "RMSDP", "MAXDP", "DIISERR"):      # calc:187-190, applied over the named criteria at calc:491-494
            custom[{"ECONV": "delta_E", "RMSDP": "RMS_DP", "MAXDP": "max_DP", "DIISERR": "commutator"}[p]] = float(value())
        elif p in ("SADGUESS", "SCFGUESS", "T", "P", "DEBUG"):
            pass                                             # (SCFGUESS: the reference's default guess path, calc:405-421 -- reproduced by default)
        else:
            raise TunaError(f"Keyword \"{p}\" is not supported on the GPU hot path (SCF keywords only)")
    # calc:473-494: first the named criteria -- a derivative request without LOOSE..EXTREME tightens them (polarisabilities: extreme,
    # dipole: tight) -- then ECONV / RMSDP / MAXDP / DIISERR are applied over whichever set was chosen
    if not any(p in params for p in ("LOOSE", "MEDIUM", "TIGHT", "EXTREME")):
        if calc.polarisability or calc.hyperpolarisability:
            calc.SCF_conv = SCF_CONVERGENCE["extreme"]
        elif calc.dipole:
            calc.SCF_conv = SCF_CONVERGENCE["tight"]
    if custom:
        calc.SCF_conv = dict(calc.SCF_conv, **custom)
    return calc


def build_molecule_and_integrals(symbols, R_bohr, calc: Calculation, engine: Engine, sharded_fock_factory=None):
    """energy:770-870 for the hot path: molecule, one- and two-electron integrals (GPU), orthogonaliser, guess."""
    atoms = mol.make_atoms(symbols, R_bohr)
    shells = mol.build_shells(atoms, calc.basis, calc.decontract)
    aos = mol.expand_cartesian_aos(shells)
    spherical = not calc.cartesian_harmonics
    n_el = mol.electron_count(atoms, calc.charge)
    if n_el <= 0:
        raise TunaError("Zero electrons specified!" if n_el == 0 else "Negative number of electrons specified!")
    n_unpaired = calc.multiplicity - 1
    if calc.multiplicity < 1 or (n_el - n_unpaired) % 2 or n_unpaired > n_el:
        raise TunaError("Impossible charge and multiplicity combination!")
    n_alpha, n_beta = (n_el + n_unpaired) // 2, (n_el - n_unpaired) // 2
    if calc.multiplicity != 1:
        calc.reference = "UHF"                               # tuna_molecule.py:307
    timings = {}
    t0 = time.perf_counter()
    engine.set_basis(aos)
    xyz, chg = [a.origin for a in atoms], [float(a.charge) for a in atoms]
    from . import guess as guess_mod
    com = [0.0, 0.0, guess_mod.centre_of_mass(atoms) if len(atoms) == 2 else 0.0]     # dipole origin, kernel:312
    S, T, V, D, Q = engine.one_electron(xyz, chg, com, spherical=spherical)
    timings["One-electron integrals"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    engine.build_eri(spherical=spherical)
    timings["Two-electron integrals"] = time.perf_counter() - t0
    fock = sharded_fock_factory(engine) if sharded_fock_factory is not None and engine.world > 1 else None
    integrals = Integrals(S, T, V, D, Q, DeviceERI(engine, fock))
    if calc.functional is not None:                         # Kohn-Sham: grid + AOs on the grid (tuna_dft.py:94-208)
        from . import dft as dft_mod
        t0 = time.perf_counter()
        pts, wts, ginfo = dft_mod.integration_grid(atoms, calc.grid_conv)
        f = engine.dft_setup(pts, wts, calc.functional, calc.X_alpha)
        calc.HFX_prop, calc.DFT_calculation = f["hfx"], True
        timings["Integration grid setup"] = time.perf_counter() - t0
    else:
        engine.dft_clear()
    dim = (lambda s: s.n_sph) if spherical else (lambda s: s.n_cart)
    ranges = [sum(dim(s) for s in shells if s.atom == a) for a in range(len(atoms))]
    molecule = Molecule(atoms, shells, aos, n_el, n_el // 2, n_alpha, n_beta, ranges, engine.N, aos.n)
    t0 = time.perf_counter()
    X, smallest, S_inv = engine.orthogonaliser(S)
    timings["Fock orthogonalisation matrix"] = time.perf_counter() - t0
    if smallest < calc.S_eigenvalue_threshold:            # STHRESH, kernel:887
        raise TunaError("An overlap matrix eigenvalue is too small! Change the basis set or decrease the threshold with STHRESH.")
    t0 = time.perf_counter()
    use_core = calc.core_guess or calc.cartesian_harmonics or any(a.charge == 0 for a in atoms)
    if use_core:
        _, C0 = engine.diagonalise(integrals.H_core, X)
        if calc.reference == "UHF":
            Pa0, Pb0 = construct_density_matrix(C0, n_alpha, 1), construct_density_matrix(C0, n_beta, 1)
            P0 = Pa0 + Pb0
        else:
            P0 = construct_density_matrix(C0, molecule.n_doubly_occ, 2)
            Pa0 = Pb0 = P0 / 2
        E0 = float(np.einsum("mn,mn->", integrals.H_core, P0))     # guess energy, tuna_guess.py:429
    else:
        P0, Pa0, Pb0, E0 = guess_mod.superposition_guess(engine, atoms, S, S_inv, engine.sph_matrix(), n_alpha, n_beta, integrals.H_core)
    timings["Initial guess"] = time.perf_counter() - t0
    return molecule, integrals, X, (P0, Pa0, Pb0, E0), timings


def calculate_energy(symbols, R_bohr, calc: Calculation, engine: Engine | None = None, silent=True, log=print):
    if calc.triples and calc.coupled_cluster not in ("CCSD", "QCISD"):
        raise TunaError(f"Perturbative triples follow CCSD or QCISD only, not {calc.coupled_cluster or calc.method}!")
    own = engine is None
    engine = engine or Engine(0)
    try:
        molecule, integrals, X, guess, timings = build_molecule_and_integrals(symbols, R_bohr, calc, engine)
        V_NN = mol.nuclear_repulsion(molecule.atoms)
        # field terms of the Hamiltonian, set after the guess as the reference does (energy:915-919; kernel:660-707: only two
        # independent components of the quadrupole tensor are used, [Q0, Q0, Q1])
        if np.linalg.norm(calc.electric_field) > 0:
            integrals.F = np.einsum("i,ijk->jk", np.asarray(calc.electric_field, dtype=float), integrals.D, optimize=True)
        if np.linalg.norm(calc.electric_field_gradient) > 0:
            Q3 = np.array([integrals.Q[0], integrals.Q[0], integrals.Q[1]])
            integrals.G = np.einsum("i,ijk->jk", np.asarray(calc.electric_field_gradient, dtype=float), Q3, optimize=True)
        if not silent:
            log(f" Nuclear repulsion energy: {V_NN:.10f}\n")
        t0 = time.perf_counter()
        out = run_self_consistent_field_cycle(molecule, calc, integrals, V_NN, X, guess, None, silent, log)
        timings["Self-consistent field"] = time.perf_counter() - t0
        out.timings.update(timings)
        if not silent:
            if calc.functional is not None and calc.reference == "UHF":
                space = " " * max(0, 8 - len(calc.functional))
                log(f"\n Unrestricted {calc.functional} energy: {space}    " + f"{out.energy:16.10f}")   # kernel:856-858
            elif calc.functional is not None:
                space = " " * max(0, 8 - len(calc.functional))
                log(f"\n Restricted {calc.functional} energy: {space}      " + f"{out.energy:16.10f}")     # kernel:854
            else:
                label = "\n Unrestricted Hartree-Fock energy: " if calc.reference == "UHF" else "\n Restricted Hartree-Fock energy:   "
                log(label + f"{out.energy:16.10f}")                                      # kernel:846-850
        if calc.stability_analysis:                          # after the SCF's energy components, before any post-SCF stage (kernel:1144-1148)
            if kohn_sham_kernel_available(calc):
                run_kohn_sham_stability(calc, molecule, out, engine, silent, log)
            else:
                run_stability_analysis(calc, molecule, out, engine, silent, log)
        if calc.method == "MP2" and calc.mp4:
            run_restricted_mp4(calc, molecule, out, engine, silent, log)
        elif calc.method == "MP2":
            # second-order Moller-Plesset correlation energy on the device-resident tensor (all-electron, SURVEY.md section 8d
            # config 5): restricted, AO->MO of the (ia|jb) block + the energy sums, tf_mp2_rhf (tuna_mp.py:834-906); unrestricted, the
            # three spin blocks, tf_mp2_uhf (tuna_mp.py:987-1117)
            t0 = time.perf_counter()
            if calc.reference == "UHF":
                r = engine.mp2_uhf(out.molecular_orbitals_alpha, out.molecular_orbitals_beta, out.epsilons_alpha, out.epsilons_beta,
                                   molecule.n_alpha, molecule.n_beta)
            elif calc.mp3:
                # MP3 / SCS-MP3 (tuna_mp.py:1418-1493): tf_mp3_rhf returns the MP2 components of the same orbitals as well
                r3 = engine.mp3_rhf(out.molecular_orbitals, out.epsilons, molecule.n_doubly_occ, 0)
                r = {k: r3[k] for k in ("E_OS", "E_SS", "E_MP2", "seconds")}
            else:
                r = engine.mp2_rhf(out.molecular_orbitals, out.epsilons, molecule.n_doubly_occ, 0)
            out.timings["MP2 energy"] = time.perf_counter() - t0
            E_SS, E_OS = r["E_SS"], r["E_OS"]
            if calc.spin_component_scaling:                  # mp:474-503
                E_SS, E_OS = calc.same_spin_scaling * E_SS, calc.opposite_spin_scaling * E_OS
                r = dict(r, E_SS=E_SS, E_OS=E_OS, E_MP2=E_SS + E_OS)
                if not silent:
                    log(f"  Same-spin scaling: {calc.same_spin_scaling:.3f}")
                    log(f"  Opposite-spin scaling: {calc.opposite_spin_scaling:.3f}\n")
            out.mp2 = r
            E_SCF = out.energy
            out.correlation_energy_mp2 = r["E_MP2"]
            out.energy = E_SCF + r["E_MP2"]
            if not silent:
                if calc.reference == "UHF":
                    log(f"  Energy from alpha-alpha pairs:      {r['E_aa']:13.10f}")     # mp:1111-1117
                    log(f"  Energy from beta-beta pairs:        {r['E_bb']:13.10f}")
                    log(f"  Energy from alpha-beta pairs:       {r['E_ab']:13.10f}")
                    log(f"\n  Same spin contribution:             {E_SS:13.10f}")
                else:
                    log(f"\n  Same spin contribution:             {E_SS:13.10f}")       # mp:904-906
                log(f"  Opposite spin contribution:         {E_OS:13.10f}")
                log(f"\n  MP2 correlation energy:             {r['E_MP2']:13.10f}")
            if mp2_density_requested(calc):
                run_mp2_density(calc, molecule, integrals, X, out, engine, silent, log)
            if calc.mp3:
                E_MP3 = r3["E_MP3"]
                if not silent:
                    log(f"\n  MP3 correlation energy:             {E_MP3:13.10f}")                  # mp:1472
                if calc.spin_component_scaling:                                                    # mp:1476-1482
                    E_MP3 *= calc.MP3_scaling
                    if not silent:
                        log(f"\n  Scaling for MP3: {calc.MP3_scaling:.3f}\n")
                        log(f"  Scaled MP3 correlation energy:    {E_MP3:15.10f}")
                        log(f"  SCS-MP3 correlation energy:       {(E_MP3 + r['E_MP2']):15.10f}")
                out.mp3 = dict(r3, E_MP3_scaled=E_MP3)
                out.correlation_energy_mp3 = E_MP3
                out.energy += E_MP3
                if not silent:                                                                     # kernel:1223-1239
                    tag = "SCS-" if calc.spin_component_scaling else ""
                    log(f"\n Correlation energy from {tag}MP2:  {' ' * (4 - len(tag))}" + f"{r['E_MP2']:16.10f}")
                    log(f" Correlation energy from {tag}MP3:  {' ' * (4 - len(tag))}" + f"{E_MP3:16.10f}\n")
                    log(" Total correlation energy:         " + f"{r['E_MP2'] + E_MP3:16.10f}\n")
        if calc.coupled_cluster in CCSD_METHODS:
            run_coupled_cluster_singles_doubles(calc, molecule, out, engine, silent, log)
            if calc.triples:
                run_perturbative_triples(calc, molecule, out, engine, silent, log)
        elif calc.coupled_cluster:
            run_coupled_cluster_doubles(calc, molecule, out, engine, silent, log)
        if calc.excited_state and calc.reference == "UHF" and kohn_sham_kernel_available(calc):
            run_unrestricted_tddft(calc, molecule, integrals, out, engine, silent, log)
        elif calc.excited_state:
            run_excited_states(calc, molecule, integrals, out, engine, silent, log)
        if not silent:
            log(" Final single point energy:        " + f"{out.energy:16.10f}")        # kernel:1305
            if getattr(out, "mp2_density_type", None):
                log(f"\n Using the MP2 {out.mp2_density_type} density for property calculations.")     # tuna_props.py:826
        if calc.dipole or calc.polarisability or calc.hyperpolarisability:
            # finite-field properties (energy:941-957): the cycles of a property run in lockstep on the resident tensor
            from . import properties as props
            if calc.method == "MP2" or calc.coupled_cluster:
                raise TunaError("finite-field properties are available for Hartree-Fock energies in this build")
            t0 = time.perf_counter()
            fe = props.FieldEnergies(molecule, calc, integrals, V_NN, X, guess)
            out.properties = {}
            if calc.dipole:
                out.properties["dipole_moment"] = props.calculate_numerical_dipole_moment(fe, silent, log)
            if calc.polarisability:
                out.properties["polarisability"] = props.calculate_polarisability(fe, out.energy, silent, log)
            if calc.hyperpolarisability:
                out.properties["hyperpolarisability"] = props.calculate_hyperpolarisability(fe, silent, log)
            out.timings["Electric properties"] = time.perf_counter() - t0
        out.integrals = integrals if not own else None      # the device tensor dies with an engine we own
        return out
    finally:
        if own:
            engine.close()


def frozen_core_orbitals(molecule, calc: Calculation) -> int:
    """The frozen orbitals of either spin: 0 unless calc.freeze_core, else the sum over the atoms of 0 (H - Be), 1 (B - Mg), 5 (Al - Ar),
    the counts the reference's atomic data holds (tuna_molecule.py:332)."""
    if not calc.freeze_core:
        return 0
    n = sum(0 if a.charge <= 4 else (1 if a.charge <= 12 else 5) for a in molecule.atoms)
    if 2 * n > molecule.n_electrons:
        raise TunaError("Not enough spatial orbitals to freeze!")                         # tuna_ci.py:547, :652
    return n


def run_stability_analysis(calc: Calculation, molecule, out, engine: Engine, silent=True, log=print):
    """STAB: determine_self_consistent_field_stability (tuna_ci.py:1049-1106) for a Hartree-Fock SCF, tf_stability_rhf / tf_stability_uhf:
    the lowest eigenvalues of the orbital Hessian [[A, B], [B, A]] from eig(A + B) and eig(A - B) -- singlet and triplet for RHF,
    spin-conserving for UHF -- with the reference's block (:946-983, :1014-1036, :1092-1106) and its threshold of -1e-5.  out.stability
    holds the eigenvalues, which matrix each came from, the verdicts and the seconds.  An unstable solution is reported, not raised."""
    if calc.functional is not None:
        raise TunaError("STAB: the stability analysis of a Kohn-Sham solution (the orbital Hessian with the exchange-correlation kernel) is "
                        "not built: STAB is available on Hartree-Fock references (HF, UHF, and the correlated methods on them).")
    _stability_analysis(calc, molecule, out, engine, silent, log, False)


def kohn_sham_kernel_available(calc: Calculation) -> bool:
    """A Kohn-Sham Calculation whose functional has an exchange-correlation kernel in this build (tuna_amd.dft.TD_AVAILABLE)"""
    from . import dft as dft_mod
    return calc.functional is not None and calc.functional in dft_mod.TD_AVAILABLE


def run_kohn_sham_stability(calc: Calculation, molecule, out, engine: Engine, silent=True, log=print):
    """STAB on a Kohn-Sham solution of a functional of tuna_amd.dft.TD_AVAILABLE, restricted or unrestricted
    (determine_self_consistent_field_stability with K_XC_singlet / K_XC_triplet / K_XC, tuna_ci.py:1049-1106): tf_stability_rks /
    tf_stability_uks with calc.HFX_prop at the SCF densities, on the grid the Kohn-Sham SCF left on the engine.  Prints the three lines of
    the kernel build (tuna_dft.py:1099-1181, :1221-1254), then the reference's block with its threshold; out.stability as
    run_stability_analysis.  Reached through calculate_energy with a Calculation; the input lines stay refused by run()."""
    if not kohn_sham_kernel_available(calc):
        raise TunaError("Stability analysis is not yet available for this exchange-correlation functional!")       # tuna_ci.py:1072
    _stability_analysis(calc, molecule, out, engine, silent, log, True)


def _stability_analysis(calc: Calculation, molecule, out, engine: Engine, silent, log, ks):
    N = molecule.n_basis
    threshold = ORB_HESS_EIG_THRESH
    nf = frozen_core_orbitals(molecule, calc)
    t0 = time.perf_counter()
    if calc.reference == "UHF":
        if (molecule.n_alpha - nf) * (N - molecule.n_alpha) + (molecule.n_beta - nf) * (N - molecule.n_beta) <= 0:
            raise TunaError("Stability analysis requested on system with no orbital rotations!")
        if ks:
            r = engine.stability_uks(out.molecular_orbitals_alpha, out.molecular_orbitals_beta, out.epsilons_alpha, out.epsilons_beta, out.P_alpha,
                                     out.P_beta, molecule.n_alpha, molecule.n_beta, nf, nf, hfx=calc.HFX_prop)
        else:
            r = engine.stability_uhf(out.molecular_orbitals_alpha, out.molecular_orbitals_beta, out.epsilons_alpha, out.epsilons_beta, molecule.n_alpha,
                                     molecule.n_beta, nf, nf)
        lowest = r["lowest"]
        st = {"reference": "UHF", "lowest": lowest, "source": r["source"], "unstable_unrestricted": lowest <= threshold, "stable": lowest > threshold}
    else:
        if N - molecule.n_doubly_occ <= 0:
            raise TunaError("Stability analysis requested on system with no orbital rotations!")
        if ks:
            r = engine.stability_rks(out.molecular_orbitals, out.epsilons, out.P, molecule.n_doubly_occ, nf, hfx=calc.HFX_prop)
        else:
            r = engine.stability_rhf(out.molecular_orbitals, out.epsilons, molecule.n_doubly_occ, nf)
        ls, lt = r["lowest_singlet"], r["lowest_triplet"]
        st = {"reference": "RHF", "lowest_singlet": ls, "lowest_triplet": lt, "source_singlet": r["source_singlet"], "source_triplet": r["source_triplet"],
              "unstable_restricted": ls <= threshold, "unstable_unrestricted": lt <= threshold, "stable": ls > threshold and lt > threshold}
    out.timings["Stability analysis"] = time.perf_counter() - t0
    st.update(threshold=threshold, dim=r["dim"], n_frozen=nf, seconds=r["seconds"])
    out.stability = st
    if silent:
        return
    if ks:
        log("\n Evaluating molecular orbitals on grid...    [Done]")
        log(" Evaluating exchange-correlation kernel...   [Done]")
        log(" Calculating matrix elements...              [Done]")
    log("\n" + SPACER)
    log("                  Stability Analysis")
    log(SPACER)
    if calc.reference == "UHF":
        log("  Building unrestricted orbital Hessian...   [Done]")
        log("\n  Diagonalising orbital Hessian...           [Done]")
        log(f"\n  Lowest Hessian eigenvalue:             {st['lowest']:10.5f}")
        if st["unstable_unrestricted"]:
            log("\n  The SCF is unstable wrt. unrestricted rotations.")
        else:
            log("\n  The self-consistent field solution is stable!")
    else:
        log("  Building singlet orbital Hessian...        [Done]")
        log("  Building triplet orbital Hessian...        [Done]")
        log("\n  Diagonalising orbital Hessians...          [Done]")
        log(f"\n  Lowest singlet eigenvalue:             {st['lowest_singlet']:10.5f}")
        log(f"  Lowest triplet eigenvalue:             {st['lowest_triplet']:10.5f}")
        if st["unstable_restricted"]:
            log("\n  The SCF is unstable wrt. restricted rotations.")
        if st["unstable_unrestricted"]:
            log("\n  The SCF is unstable wrt. unrestricted rotations.")
        if st["stable"]:
            log("\n  The self-consistent field solution is stable!")
    log(SPACER)


def mp2_density_requested(calc: Calculation) -> bool:
    return calc.relaxed_density or calc.unrelaxed_density or calc.natural_orbitals


def run_mp2_density(calc: Calculation, molecule, integrals, X, out, engine: Engine, silent=True, log=print):
    """The MP2 one-particle density after a restricted MP2 / SCS-MP2 energy (all-electron), tf_mp2_density_rhf and tf_natural_orbitals:
    the density part of run_restricted_MP2 (tuna_mp.py:908-973) -- unrelaxed unless RELAXED asks for the Z-vector relaxed one, the
    SCS weights on both spin parts -- then calculate_natural_orbitals (:514-565; its block is printed with NATORBS, as there) and the
    analytical dipole moment about the centre of mass (tuna_props.py:96-121).  out.P, out.P_alpha and out.P_beta become the MP2 density."""
    from . import guess as guess_mod
    relaxed = calc.relaxed_density
    density_type = "relaxed" if relaxed else "unrelaxed"
    c_os, c_ss = (calc.opposite_spin_scaling, calc.same_spin_scaling) if calc.spin_component_scaling else (1.0, 1.0)
    t0 = time.perf_counter()
    d = engine.mp2_density_rhf(out.molecular_orbitals, out.epsilons, molecule.n_doubly_occ, 0, relaxed=relaxed, c_os=c_os, c_ss=c_ss)
    occ, orbitals = engine.natural_orbitals(d["P_ao"], X)
    out.timings["MP2 density"] = time.perf_counter() - t0
    if not silent:
        pad = "   " if relaxed else " "
        log(f"\n  Constructing MP2 {density_type} density...{pad}     [Done]")                        # mp:910-914, :967
        if calc.natural_orbitals:                                                                  # mp:551-562
            log("")
            log("  Natural orbital occupancies: \n")
            for k, n in enumerate(occ):
                log(f"    {(k + 1):2.0f}. {n:12.8f}")
            log(f"\n  Sum of natural orbital occupancies: {np.sum(occ):.6f}")
            log(f"  Trace of density matrix: {np.sum(occ):.6f}")
    out.P, out.P_alpha, out.P_beta = d["P_ao"], d["P_ao"] / 2, d["P_ao"] / 2
    out.mp2 = dict(out.mp2, P_mo=d["P_mo"], L=d["L"], z=d["z"], density_seconds=d["seconds"])
    out.mp2_density_type = density_type
    out.natural_orbital_occupancies, out.natural_orbitals = occ, orbitals
    atoms = molecule.atoms
    com = guess_mod.centre_of_mass(atoms) if len(atoms) == 2 else 0.0
    nuclear = float(sum((a.origin[2] - com) * float(a.charge) for a in atoms))
    electronic = -float(np.einsum("ij,ij->", d["P_ao"], integrals.D[2], optimize=True))
    out.properties = dict(getattr(out, "properties", None) or {}, dipole_moment=(nuclear + electronic, nuclear, electronic))


def run_restricted_mp4(calc: Calculation, molecule, out, engine: Engine, silent=True, log=print):
    """Restricted MP4(SDQ) / MP4(DQ) on the device-resident tensor (all-electron), tf_mp4_rhf, which returns the MP2 and MP3 parts of the
    same orbitals as well: the log lines of run_restricted_MP2 (tuna_mp.py:904-906), run_restricted_MP3 (:1472), run_restricted_MP4
    (:1576-1682) and the summary of tuna_kernel.py:1245-1262.  Nothing is scaled: out.energy = E_SCF + E_MP2 + E_MP3 + E_MP4.
    Level "SDTQ" is full MP4: tf_mp4_rhf at level SDQ, then the triples of tf_triples_rhf (kind MP4), E_MP4 = E_S + E_D + E_T + E_Q."""
    level = calc.mp4
    full = level == "SDTQ"
    t0 = time.perf_counter()
    r = engine.mp4_rhf(out.molecular_orbitals, out.epsilons, molecule.n_doubly_occ, 0, level="SDQ" if full else level)
    if full:
        out.triples = engine.triples_rhf(out.molecular_orbitals, out.epsilons, molecule.n_doubly_occ, 0, kind="MP4")
        out.correlation_energy_triples = out.triples["E_T"]
        r = dict(r, E_T=out.triples["E_T"], E_MP4=r["E_S"] + r["E_D"] + out.triples["E_T"] + r["E_Q"])
    out.timings["MP4 energy" if full else f"MP4({level}) energy"] = time.perf_counter() - t0
    E_MP2, E_MP3, E_MP4 = r["E_MP2"], r["E_MP3"], r["E_MP4"]
    if not silent:
        log(f"\n  Same spin contribution:             {r['E_SS']:13.10f}")              # mp:904-906
        log(f"  Opposite spin contribution:         {r['E_OS']:13.10f}")
        log(f"\n  MP2 correlation energy:             {E_MP2:13.10f}")
        log(f"\n  MP3 correlation energy:             {E_MP3:13.10f}")                  # mp:1472
        log("                      MP4 Energy  ")                                       # mp:1577
        if level == "SDQ":                                                              # mp:1665-1675
            log("  Triples are not included in MP4(SDQ).\n")
        elif full:
            log("  Triples are included in full MP4.\n")
        else:
            log("  Singles and triples are not included in MP4(DQ).\n")
        log(f"  Singles correlation energy:         {r['E_S']:13.10f}")                 # mp:1677-1682
        log(f"  Doubles correlation energy:         {r['E_D']:13.10f}")
        log(f"  Triples correlation energy:         {r['E_T'] if full else 0.0:13.10f}")
        log(f"  Quadruples correlation energy:      {r['E_Q']:13.10f}")
        log(f"\n  MP4 correlation energy:             {E_MP4:13.10f}")
        log("\n Correlation energy from MP2:      " + f"{E_MP2:16.10f}")                # kernel:1247-1262
        log(" Correlation energy from MP3:      " + f"{E_MP3:16.10f}")
        if full:
            log(" Correlation energy from MP4:      " + f"{E_MP4:16.10f}\n")
        else:
            log(f" Correlation energy from MP4({level}):{' ' * (4 - len(level))}" + f"{E_MP4:16.10f}\n")
        log(" Total correlation energy:         " + f"{E_MP2 + E_MP3 + E_MP4:16.10f}\n")
    out.mp2 = {k: r[k] for k in ("E_OS", "E_SS", "E_MP2", "seconds")}
    out.mp3 = dict({k: r[k] for k in ("E_OS", "E_SS", "E_MP2", "E_pp", "E_hh", "E_ring", "E_MP3", "seconds")}, E_MP3_scaled=E_MP3)
    out.mp4 = r
    out.correlation_energy_mp2, out.correlation_energy_mp3, out.correlation_energy_mp4 = E_MP2, E_MP3, E_MP4
    out.energy += E_MP2 + E_MP3 + E_MP4


def run_coupled_cluster_doubles(calc: Calculation, molecule, out, engine: Engine, silent=True, log=print):
    """Restricted LCCD / CCD on the device-resident tensor (all-electron), tf_ccd_rhf: the iteration of calculate_coupled_cluster_energy
    (tuna_cc.py:2950-3175) with its log lines (tuna_cc.py:163-199, :3139, :3164-3170; kernel:1282).  The energy threshold is the chosen
    SCF set's delta_E, or ECONV (calc:518)."""
    name = calc.coupled_cluster
    conv_E = calc.SCF_conv["delta_E"]
    t0 = time.perf_counter()
    r = engine.ccd_rhf(out.molecular_orbitals, out.epsilons, molecule.n_doubly_occ, 0, method=name, max_iter=calc.correlated_max_iter,
                       conv_delta_E=conv_E, conv_amplitudes=calc.amp_conv, use_diis=calc.DIIS, max_diis=calc.max_DIIS_matrices,
                       damping=calc.correlated_damping_parameter, allow_unconverged=True)
    out.timings[f"{name} energy"] = time.perf_counter() - t0
    if not silent:
        log(f"              {name:>5} Energy and Density ")
        log(f"  Energy convergence tolerance:        {conv_E:.10f}")
        log(f"  Amplitude convergence tolerance:     {calc.amp_conv:.10f}")
        log(f"\n  Guess t-amplitude MP2 energy:       {r['E_MP2']:.10f}\n")
        if calc.correlated_damping_parameter != 0:
            log(f"  Using damping parameter of {calc.correlated_damping_parameter:.2f} for convergence.")
        if calc.DIIS:
            log(f"  Using DIIS, storing {calc.max_DIIS_matrices} matrices, for convergence.")
        log(f"\n  Starting {name} iterations...\n")
        log("  Step          Correlation E               DE")
        for step, E, dE in r["table"]:
            log(f"  {step:3.0f}           {E:13.10f}         {dE:13.10f}")
    if not r["converged"]:
        raise TunaError(f"The {name} iterations failed to converge! Try increasing the maximum iterations with CORRMAXITER?", -4)
    E_CC = r["E_corr"]
    if not silent:
        log(f"\n  Singles contribution:               {0.0:13.10f}")
        log(f"  Connected doubles contribution:     {E_CC:13.10f}")
        log(f"  Disconnected doubles contribution:  {0.0:13.10f}")
        log(f"\n  {name} correlation energy:  {' ' * (10 - len(name))}    {E_CC:.10f}")
        log(f" Correlation energy from {name}:{' ' * max(0, 8 - len(name))} " + f"{E_CC:16.10f}\n")
    out.cc = r
    out.correlation_energy_cc = E_CC
    out.energy += E_CC


CCSD_METHODS = ("LCCSD", "QCISD", "CCSD")


def run_coupled_cluster_singles_doubles(calc: Calculation, molecule, out, engine: Engine, silent=True, log=print):
    """Restricted LCCSD / QCISD / CCSD on the device-resident tensor (all-electron), tf_ccsd_rhf: the iteration of
    calculate_coupled_cluster_energy (tuna_cc.py:2950-3175) with its log lines (tuna_cc.py:163-199, :3139, :3164-3170), the T1 lines of
    calculate_T1_diagnostic (:670-671) and the summary line of run_coupled_cluster_doubles.  Thresholds as there.  With calc.triples the
    converged amplitudes come back as well, for run_perturbative_triples."""
    name = calc.coupled_cluster
    conv_E = calc.SCF_conv["delta_E"]
    t0 = time.perf_counter()
    amplitudes = dict(return_t1=True, return_t2=True) if calc.triples else {}
    r = engine.ccsd_rhf(out.molecular_orbitals, out.epsilons, molecule.n_doubly_occ, 0, method=name, max_iter=calc.correlated_max_iter,
                        conv_delta_E=conv_E, conv_amplitudes=calc.amp_conv, use_diis=calc.DIIS, max_diis=calc.max_DIIS_matrices,
                        damping=calc.correlated_damping_parameter, allow_unconverged=True, **amplitudes)
    out.timings[f"{name} energy"] = time.perf_counter() - t0
    if not silent:
        log(f"              {name:>5} Energy and Density ")
        log(f"  Energy convergence tolerance:        {conv_E:.10f}")
        log(f"  Amplitude convergence tolerance:     {calc.amp_conv:.10f}")
        log(f"\n  Guess t-amplitude MP2 energy:       {r['E_MP2']:.10f}\n")
        if calc.correlated_damping_parameter != 0:
            log(f"  Using damping parameter of {calc.correlated_damping_parameter:.2f} for convergence.")
        if calc.DIIS:
            log(f"  Using DIIS, storing {calc.max_DIIS_matrices} matrices, for convergence.")
        log(f"\n  Starting {name} iterations...\n")
        log("  Step          Correlation E               DE")
        for step, E, dE in r["table"]:
            log(f"  {step:3.0f}           {E:13.10f}         {dE:13.10f}")
    if not r["converged"]:
        raise TunaError(f"The {name} iterations failed to converge! Try increasing the maximum iterations with CORRMAXITER?", -4)
    E_CC = r["E_corr"]
    if not silent:
        log(f"\n  Singles contribution:               {r['E_singles']:13.10f}")
        log(f"  Connected doubles contribution:     {r['E_connected']:13.10f}")
        log(f"  Disconnected doubles contribution:  {r['E_disconnected']:13.10f}")
        log(f"\n  {name} correlation energy:  {' ' * (10 - len(name))}    {E_CC:.10f}")
        log(f"\n  Norm of singles amplitudes:         {r['t1_norm']:13.10f}")
        log(f"  Value of T1 diagnostic:             {r['T1_diagnostic']:13.10f}")
        log(f" Correlation energy from {name}:{' ' * max(0, 8 - len(name))} " + f"{E_CC:16.10f}\n")
    out.cc = r
    out.correlation_energy_cc = E_CC
    out.energy += E_CC


def run_perturbative_triples(calc: Calculation, molecule, out, engine: Engine, silent=True, log=print):
    """CCSD(T) / QCISD(T) after run_coupled_cluster_singles_doubles (all-electron), tf_triples_rhf on the converged amplitudes of out.cc:
    the section of calculate_restricted_CCSD_T_energy (tuna_cc.py:2713-2756; QCISD(T) prints one space less, as there) and the summary
    lines of tuna_kernel.py:1276-1278.  The line " Correlation energy from CCSD:" of the singles-doubles step stays where that step prints
    it, in front of this section; the summary repeats it in the reference's format.  out.energy grows by E_T."""
    name = f"{calc.coupled_cluster}(T)"
    t0 = time.perf_counter()
    r = engine.triples_rhf(out.molecular_orbitals, out.epsilons, molecule.n_doubly_occ, 0, kind=name, t1=out.cc["t1"], t2=out.cc["t2"])
    out.timings[f"{name} energy"] = time.perf_counter() - t0
    E_CC, E_T = out.correlation_energy_cc, r["E_T"]
    if not silent:
        space = "" if "QCISD" in name else " "                                          # cc:2733-2740
        log(f"                    {name} Energy ")                                       # cc:2714
        log("  Forming disconnected amplitudes...         [Done]")                      # cc:2725, :2742
        log("  Forming connected amplitudes...            [Done]")                      # cc:2744, :2750
        log(f"\n  Calculating {name} correlation energy... {space}[Done]\n")           # cc:2752, :2756
        log(f"  {name} correlation energy:       {space} {E_T:13.10f}")
        space = " " * max(0, 8 - len(name))                                             # kernel:1272-1278
        log(f" Correlation energy from {calc.coupled_cluster}:{space}    {E_CC:16.10f}")
        log(f" Correlation energy from {name}: {space}{E_T:16.10f}\n")
        log(f" Total correlation energy: {space}       {E_CC + E_T:16.10f}\n")
    out.triples = r
    out.correlation_energy_triples = E_T
    out.energy += E_T


ORB_HESS_EIG_THRESH = -1e-5                                                                      # tuna_util.py:103
_HARTREE_IN_JOULES = (mol._hbar ** 2) / (mol._me * mol.BOHR_IN_METRES ** 2)                       # tuna_util.py:53
PER_CM_IN_HARTREE = _HARTREE_IN_JOULES / (299792458 * mol._h * 10 ** 2)                          # tuna_util.py:60
EV_IN_HARTREE = _HARTREE_IN_JOULES / mol._e                                                      # tuna_util.py:63


def merge_excited_states(E_singlet, E_triplet, tdm_singlet=None, osc_singlet=None):
    """The merged list of run_excited_state_calculation (tuna_ci.py:2209-2267): singlets then triplets, sorted by energy with a stable
    sort.  Returns (energies, labels, source index within the multiplicity, |mu|, f); triplets have |mu| = f = 0."""
    parts = [(np.asarray(e, dtype=float), label) for e, label in ((E_singlet, "singlet"), (E_triplet, "triplet")) if e is not None]
    energies = np.concatenate([e for e, _ in parts])
    labels = np.concatenate([np.full(len(e), label) for e, label in parts])
    source = np.concatenate([np.arange(len(e)) for e, _ in parts])
    ns = len(E_singlet) if E_singlet is not None else 0
    mu, f = np.zeros(len(energies)), np.zeros(len(energies))
    if ns and tdm_singlet is not None:
        mu[:ns] = np.linalg.norm(np.asarray(tdm_singlet, dtype=float).reshape(ns, -1), axis=1)
        f[:ns] = np.asarray(osc_singlet, dtype=float)
    order = np.argsort(energies)                             # (the reference's own call: tuna_ci.py:2263)
    return energies[order], labels[order], source[order], mu[order], f[order]


def run_excited_states(calc: Calculation, molecule, integrals, out, engine: Engine, silent=True, log=print):
    """Closed-shell CIS / TDHF on the device-resident tensor (all-electron), tf_cis_rhf -- and, when calc.functional is one of
    tuna_amd.dft.TD_AVAILABLE, TD-DFT / TDA with the exchange-correlation kernel at the SCF density out.P, tf_tddft_rhf with
    calc.HFX_prop, on the grid the Kohn-Sham SCF left on the engine: the flow of run_excited_state_calculation
    (tuna_ci.py:2150-2290; kernel:1175-1190, :1289-1301) with its log lines (tuna_ci.py:1222-1273, :1324-1362, :1736-1863).  All states of
    the requested multiplicities are merged and sorted; out.energy = E_SCF + the excitation energy of ROOT; out.excited holds the
    merged energies, labels, |mu|, oscillator strengths, the root's X and Y and E_transition.  The root's difference density (P_diff of
    determine_restricted_excited_state_energy_and_density) and properties on it are not formed in this build.  With
    calc.do_perturbative_doubles the root gets its CIS(D) correction after the spectrum (run_perturbative_doubles).  A TDHF run on an
    unstable reference raises the library's TunaError (TF_ELINALG) where the reference warns and drops states."""
    if calc.reference == "UHF":
        if calc.functional is not None:
            raise TunaError("Unrestricted time-dependent DFT is not built: TD-DFT runs on a closed-shell restricted Kohn-Sham reference.")
        return run_unrestricted_excited_states(calc, molecule, integrals, out, engine, silent, log)
    n_occ, N = molecule.n_doubly_occ, molecule.n_basis
    v = N - n_occ
    if calc.calculate_no_singlets and calc.calculate_no_triplets:
        raise TunaError("There are no excited states to calculate!")                      # tuna_ci.py:2171
    if v <= 0:
        raise TunaError("Excited state calculation requested on system with no virtual orbitals!")   # kernel:1181
    tda = calc.tamm_dancoff_approximation
    ks = calc.functional is not None                         # TD-DFT / TDA with the exchange-correlation kernel (tuna_ci.py:2199-2201)
    if ks:
        from . import dft as dft_mod
        if calc.functional not in dft_mod.TD_AVAILABLE:
            raise TunaError("Time-dependent DFT is not yet available for this exchange-correlation functional!")   # tuna_ci.py:2175
        if calc.do_perturbative_doubles:
            raise TunaError("The (D) correction of a TD-DFT state is not built: (D) applies to a CIS, TDHF, RPA or HF ... : TD state.")
    if not silent:
        log("\n Beginning excited state calculation...")                                  # kernel:1177
        if ks:                                                                            # tuna_dft.py:1099-1181
            log("\n Evaluating molecular orbitals on grid...    [Done]")
            log(" Evaluating exchange-correlation kernel...   [Done]")
            log(" Calculating matrix elements...              [Done]")
        log("\n" + SPACER)                                                                # tuna_ci.py:1236-1271
        log("      Time-dependent Density Functional Theory" if ks else
            "          Configuration Interaction Singles" if tda else "            Time-dependent Hartree-Fock")
        log(SPACER)
        log(("  Using" if tda else "  Not using") + " the Tamm-Dancoff approximation...\n")
        if not calc.calculate_no_triplets and not calc.calculate_no_singlets:
            log("  Singlet and triplet states will be calculated.")
        elif not calc.calculate_no_triplets:
            log("  Only triplet states will be calculated.")
        else:
            log("  Only singlet states will be calculated.")
    t0 = time.perf_counter()
    n_keep = max(calc.n_states, calc.root, 0)
    if ks:
        r = engine.tddft_rhf(out.molecular_orbitals, out.epsilons, out.P, n_occ, 0, method="TDA" if tda else "TDDFT", hfx=calc.HFX_prop,
                             singlets=not calc.calculate_no_singlets, triplets=not calc.calculate_no_triplets, n_keep=n_keep, dip=integrals.D)
    else:
        r = engine.cis_rhf(out.molecular_orbitals, out.epsilons, n_occ, 0, method="CIS" if tda else "TDHF", singlets=not calc.calculate_no_singlets,
                           triplets=not calc.calculate_no_triplets, n_keep=n_keep, dip=integrals.D)
    out.timings["Excited state calculation"] = time.perf_counter() - t0
    if not silent:
        log("\n  Building excited state Hamiltonian...      [Done]")                      # tuna_ci.py:1324-1362
        log("  Diagonalising Hamiltonian...               [Done]")
        log("\n  Calculating oscillator strengths...        [Done]")                      # tuna_ci.py:2243-2259
    energies, labels, source, mu, f = merge_excited_states(r["E_singlet"], r["E_triplet"], r["tdm"], r["osc"])
    state = calc.root - 1
    if not 0 <= state < len(energies):
        raise TunaError(f"Specified root ({state + 1}) does not exist!")                  # tuna_ci.py:1619
    if not silent:
        log("  Constructing density matrix...             [Done]")                        # tuna_ci.py:2269-2281 (the energy only, here)

    def vectors(n):
        k = int(source[n])
        return r[f"X_{labels[n]}"][k], r[f"Y_{labels[n]}"][k]
    o = n_occ
    if not silent:
        log("\n  Printing excited state information...")                                  # tuna_ci.py:1817-1861
        log(f"  Only printing contributions larger than {calc.excited_state_contribution_threshold:.1f} %.")
        for n in range(min(len(energies), calc.n_states)):
            log(f"\n  ~~~~~ State {n + 1} ~~~~~  {str(labels[n]).capitalize()}")
            log(f"\n  Excitation energy: {energies[n]:16.10f}\n")
            X, Y = vectors(n)
            contributions = 100 * (X ** 2 - Y ** 2)
            for index in np.argsort(contributions, axis=None)[::-1]:
                i, a = divmod(int(index), v)
                if contributions[i, a] <= calc.excited_state_contribution_threshold:
                    break
                log(f"    {f'{i + 1}':>4}  ->  {f'{o + a + 1}':<4}  {contributions[i, a]:7.2f} %")
        # print_excited_state_absorption_spectrum, tuna_ci.py:1754-1785
        from . import guess as guess_mod
        com = guess_mod.centre_of_mass(molecule.atoms) if len(molecule.atoms) == 2 else 0.0
        with np.errstate(divide="ignore"):
            wavelengths_nm = 1e7 / (energies * PER_CM_IN_HARTREE)
        log("\n" + SPACER)
        log(f"\n Transition dipole moment origin is the centre of mass, {com * mol.BOHR_RADIUS_IN_ANGSTROM:.4f} angstroms from the first atom.")
        log("\n" + BIG_SPACER)
        log("                                     Excited State Absorption Spectrum")
        log(BIG_SPACER)
        log("   State         Energy          Energy (eV)     Wavelength (nm)    Osc. Strength     Transition Dipole")
        log(BIG_SPACER)
        for n in range(min(len(energies), calc.n_states)):
            log(f"  {(n + 1):2} - {str(labels[n])[0].upper()}  {energies[n]:16.10f}  {EV_IN_HARTREE * energies[n]:14.5f}   {wavelengths_nm[n]:16.5f}       "
                f"{f[n]:10.5f}          {mu[n]:10.5f}")
        log(BIG_SPACER)
    X, Y = vectors(state) if state < n_keep else (None, None)
    E_transition = float(energies[state])
    out.excited = {"energies": energies, "state_types": labels, "transition_dipoles": mu, "oscillator_strengths": f, "X": X, "Y": Y,
                   "E_transition": E_transition, "root": calc.root, "method": calc.excited_state, "seconds": r["seconds"],
                   "E_singlet": r["E_singlet"], "E_triplet": r["E_triplet"], "tdm_singlet": r["tdm"]}
    out.energy = out.energy + E_transition                                                # tuna_ci.py:1642
    if calc.do_perturbative_doubles:                                                      # tuna_ci.py:2293-2295
        E_transition = run_perturbative_doubles(calc, molecule, out, engine, silent, log)
    if not silent:                                                                        # kernel:1295-1299
        log(f"\n Excitation energy is the energy difference to excited state {calc.root}.")
        log(f"\n Excitation energy from {f'{calc.excited_state}:':<11} {E_transition:15.10f}")


def spin_orbital_labels(eps_alpha, eps_beta):
    """(label of alpha orbital k, label of beta orbital k): the reference numbers the orbitals of a spin as they come in the combined
    energy order (tuna_ci.py:586-603), and within one spin that is the spin's own order: the k-th alpha orbital is "<k + 1>a"."""
    return [f"{k + 1}a" for k in range(len(eps_alpha))], [f"{k + 1}b" for k in range(len(eps_beta))]


def run_unrestricted_excited_states(calc: Calculation, molecule, integrals, out, engine: Engine, silent=True, log=print):
    """Spin-conserving CIS / TDHF of a UHF determinant on the device-resident tensor, tf_cis_uhf: the "UHF" branch of
    run_excited_state_calculation (tuna_ci.py:2215-2290) with its log lines (:1222-1257, :1416-1451, :1736-1863; no multiplicity line, no
    singlet / triplet tags, spin-orbital labels such as "3a -> 5a").  Reached through calculate_energy with reference == "UHF" and
    calc.excited_state set -- the input-line names UCIS / UTDHF / URPA stay refused by run().  Honours tamm_dancoff_approximation,
    n_states, root, excited_state_contribution_threshold and freeze_core.  out.energy = E_SCF + the excitation energy of ROOT;
    out.excited holds the energies, |mu|, oscillator strengths, the root's X and Y split by spin and E_transition.  The root's density and
    difference density are not formed, and (D) on an unrestricted state is refused.  A TDHF run on an unstable reference raises the
    library's TunaError (TF_ELINALG)."""
    _unrestricted_states(calc, molecule, integrals, out, engine, silent, log, False)


def run_unrestricted_tddft(calc: Calculation, molecule, integrals, out, engine: Engine, silent=True, log=print):
    """Spin-conserving TD-DFT / TDA of an unrestricted Kohn-Sham determinant for a functional of tuna_amd.dft.TD_AVAILABLE, tf_tddft_uhf with
    calc.HFX_prop at the SCF spin densities out.P_alpha, out.P_beta on the grid the Kohn-Sham SCF left on the engine: the "UHF" branch of
    run_excited_state_calculation with density_functional_method on (tuna_ci.py:2215-2290).  Prints the three lines of the kernel build
    (tuna_dft.py:1221-1254) and then the reference's unrestricted block; everything else as run_unrestricted_excited_states.  Reached
    through calculate_energy with reference == "UHF", a functional and calc.excited_state set; the input lines stay refused by run()."""
    if calc.reference != "UHF":
        raise TunaError("run_unrestricted_tddft needs an unrestricted Kohn-Sham reference (reference == \"UHF\").")
    if not kohn_sham_kernel_available(calc):
        raise TunaError("Time-dependent DFT is not yet available for this exchange-correlation functional!")       # tuna_ci.py:2175
    _unrestricted_states(calc, molecule, integrals, out, engine, silent, log, True)


def _unrestricted_states(calc: Calculation, molecule, integrals, out, engine: Engine, silent, log, ks):
    if calc.do_perturbative_doubles:
        raise TunaError("The (D) keyword is available for a closed-shell restricted reference only in this build: the unrestricted perturbative "
                        "doubles correction is not built.")
    N, na, nb = molecule.n_basis, molecule.n_alpha, molecule.n_beta
    nf = frozen_core_orbitals(molecule, calc)
    oa, ob, va, vb = na - nf, nb - nf, N - na, N - nb
    da, db = max(0, oa) * va, max(0, ob) * vb
    if da + db <= 0:
        raise TunaError("Excited state calculation requested on system with no virtual orbitals!")   # kernel:1181
    tda = calc.tamm_dancoff_approximation or calc.excited_state == "CIS"                  # tuna_ci.py:1401
    if not silent:
        log("\n Beginning excited state calculation...")                                  # kernel:1177
        if ks:                                                                            # tuna_dft.py:1221-1254
            log("\n Evaluating molecular orbitals on grid...    [Done]")
            log(" Evaluating exchange-correlation kernel...   [Done]")
            log(" Calculating matrix elements...              [Done]")
        log("\n" + SPACER)                                                                # tuna_ci.py:1236-1257
        log("      Time-dependent Density Functional Theory" if ks else
            "          Configuration Interaction Singles" if tda else "            Time-dependent Hartree-Fock")
        log(SPACER)
        log(("  Using" if tda else "  Not using") + " the Tamm-Dancoff approximation...\n")
    t0 = time.perf_counter()
    n_keep = max(calc.n_states, calc.root, 0)
    if ks:
        r = engine.tddft_uhf(out.molecular_orbitals_alpha, out.molecular_orbitals_beta, out.epsilons_alpha, out.epsilons_beta, out.P_alpha, out.P_beta,
                             na, nb, nf, nf, method="TDA" if tda else "TDDFT", hfx=calc.HFX_prop, n_keep=n_keep, dip=integrals.D)
    else:
        r = engine.cis_uhf(out.molecular_orbitals_alpha, out.molecular_orbitals_beta, out.epsilons_alpha, out.epsilons_beta, na, nb, nf, nf,
                           method="CIS" if tda else "TDHF", n_keep=n_keep, dip=integrals.D)
    out.timings["Excited state calculation"] = time.perf_counter() - t0
    energies = np.asarray(r["E"], dtype=float)
    mu, f = np.linalg.norm(np.asarray(r["tdm"], dtype=float).reshape(len(energies), -1), axis=1), np.asarray(r["osc"], dtype=float)
    if not silent:
        log("  Building excited state Hamiltonian...      [Done]")                        # tuna_ci.py:1416-1451
        log("  Diagonalising Hamiltonian...               [Done]")
        log("\n  Calculating oscillator strengths...        [Done]")                      # tuna_ci.py:2243-2259
    state = calc.root - 1
    if not 0 <= state < len(energies):
        raise TunaError(f"Specified root ({state + 1}) does not exist!")                  # tuna_ci.py:1696
    if not silent:
        log("  Constructing density matrix...             [Done]")                        # tuna_ci.py:2269-2281 (the energy only, here)
    labels_a, labels_b = spin_orbital_labels(out.epsilons_alpha, out.epsilons_beta)

    def split_by_spin(vec):
        return vec[:da].reshape(max(0, oa), va), vec[da:].reshape(max(0, ob), vb)
    if not silent:
        log("\n  Printing excited state information...")                                  # tuna_ci.py:1817-1861
        log(f"  Only printing contributions larger than {calc.excited_state_contribution_threshold:.1f} %.")
        for n in range(min(len(energies), calc.n_states)):
            log(f"\n  ~~~~~ State {n + 1} ~~~~~  ")
            log(f"\n  Excitation energy: {energies[n]:16.10f}\n")
            contributions = 100 * (r["X"][n] ** 2 - r["Y"][n] ** 2)
            for index in np.argsort(contributions)[::-1]:
                if contributions[index] <= calc.excited_state_contribution_threshold:
                    break
                if index < da:
                    i, a = divmod(int(index), va)
                    occ_label, virt_label = labels_a[nf + i], labels_a[na + a]
                else:
                    i, a = divmod(int(index) - da, vb)
                    occ_label, virt_label = labels_b[nf + i], labels_b[nb + a]
                log(f"    {occ_label:>4}  ->  {virt_label:<4}  {contributions[index]:7.2f} %")
        # print_excited_state_absorption_spectrum, tuna_ci.py:1754-1785, with the gaps of an unrestricted reference
        from . import guess as guess_mod
        com = guess_mod.centre_of_mass(molecule.atoms) if len(molecule.atoms) == 2 else 0.0
        with np.errstate(divide="ignore"):
            wavelengths_nm = 1e7 / (energies * PER_CM_IN_HARTREE)
        log("\n" + SPACER)
        log(f"\n Transition dipole moment origin is the centre of mass, {com * mol.BOHR_RADIUS_IN_ANGSTROM:.4f} angstroms from the first atom.")
        log("\n" + BIG_SPACER)
        log("                                     Excited State Absorption Spectrum")
        log(BIG_SPACER)
        log("   State         Energy          Energy (eV)     Wavelength (nm)    Osc. Strength     Transition Dipole")
        log(BIG_SPACER)
        for n in range(min(len(energies), calc.n_states)):
            log(f"    {(n + 1):2}    {energies[n]:16.10f}  {EV_IN_HARTREE * energies[n]:14.5f}   {wavelengths_nm[n]:16.5f}       "
                f"{f[n]:10.5f}          {mu[n]:10.5f}")
        log(BIG_SPACER)
    if state < n_keep:
        (X_alpha, X_beta), (Y_alpha, Y_beta) = split_by_spin(r["X"][state]), split_by_spin(r["Y"][state])
    else:
        X_alpha = X_beta = Y_alpha = Y_beta = None
    E_transition = float(energies[state])
    out.excited = {"energies": energies, "state_types": np.array([""] * len(energies)), "transition_dipoles": mu, "oscillator_strengths": f,
                   "X_alpha": X_alpha, "X_beta": X_beta, "Y_alpha": Y_alpha, "Y_beta": Y_beta, "E_transition": E_transition, "root": calc.root,
                   "method": calc.excited_state, "seconds": r["seconds"], "dim": r["dim"], "dim_alpha": r["dim_alpha"], "n_frozen": nf, "tdm": r["tdm"]}
    out.energy = out.energy + E_transition                                                # tuna_ci.py:1719
    if not silent:                                                                        # kernel:1295-1299
        log(f"\n Excitation energy is the energy difference to excited state {calc.root}.")
        log(f"\n Excitation energy from {f'{calc.excited_state}:':<11} {E_transition:15.10f}")


def run_perturbative_doubles(calc: Calculation, molecule, out, engine: Engine, silent=True, log=print):
    """CIS(D) of the ROOT state after run_excited_states (all-electron), tf_cis_d_rhf: run_perturbative_doubles and the section of
    calculate_restricted_doubles_correction (tuna_ci.py:2090-2139, :1899-1980) at the priorities the log shows (the eV line is priority 3).
    b = X + Y of the root, omega its excitation energy, the multiplicity from its label; out.energy and E_transition move by E_D, and
    out.excited gains E_D, E_direct and E_indirect.  The MPC / double-hybrid scaling (:1966) is not built: there are no DFT excited
    states here.  Returns the corrected excitation energy."""
    ex = out.excited
    state = calc.root - 1
    omega = ex["E_transition"]
    t0 = time.perf_counter()
    r = engine.cis_d_rhf(out.molecular_orbitals, out.epsilons, molecule.n_doubly_occ, 0, b=(ex["X"] + ex["Y"])[None], omega=[omega],
                         triplet=[int(str(ex["state_types"][state]) == "triplet")])
    out.timings["Perturbative doubles"] = time.perf_counter() - t0
    E_D = float(r["E_D"][0])
    if not silent:
        log("\n" + SPACER)                                                                # tuna_ci.py:1899-1903
        log("          Perturbative Doubles Correction")
        log(SPACER)
        log(f"  Applying doubles correction to state {state + 1} only.")
        log("\n  Building doubles amplitudes...             [Done]")                       # :1905, :1915
        log("\n  Calculating direct contribution...         [Done]")                       # :1917, :1937
        log("  Calculating indirect contribution...       [Done]")                         # :1939, :1958
        # :1960 ends its line with end = "" and the restricted function never prints its [Done]: the next line follows on the same one
        log("\n  Calculating doubles correction...         " + f"\n  Original excitation energy:       {omega:15.10f}")      # :1970
        log(f"  Correction energy from (D):       {E_D:15.10f}")
        log(f"\n  Corrected excitation energy:      {(E_D + omega):15.10f}")
        log(SPACER)
    ex.update(E_D=E_D, E_direct=float(r["E_direct"][0]), E_indirect=float(r["E_indirect"][0]), E_transition=omega + E_D,
              min_denominator=float(r["min_denominator"][0]), seconds_doubles=r["seconds"])
    out.energy = out.energy + E_D                                                         # tuna_ci.py:2135
    return omega + E_D


def run(input_line: str, silent: bool = True, engine: Engine | None = None, log=print):
    """tuna.py:345 `run(input_line, suppress_output)` for single-point restricted Hartree-Fock."""
    ctype, method, basis, symbols, R, params = parse_input(input_line)
    if ctype != "SPE":
        raise TunaError(f"Calculation type \"{ctype}\" is not supported.")
    from . import dft as dft_mod
    # a "U" prefix asks for the unrestricted reference (tuna.py:186-201): UB3LYP is B3LYP on the unrestricted cycle
    unrestricted_ks = method.startswith("U") and method[1:] in dft_mod.FUNCTIONALS
    if unrestricted_ks:
        method = method[1:]
    # UMP2 / USCS-MP2: MP2 on the unrestricted reference, as MP2 with ML n >= 2 is (tuna_mp.py:987-1222)
    unrestricted_mp2 = method in ("UMP2", "USCS-MP2")
    if unrestricted_mp2:
        method = method[1:]
    if method in ("UMP3", "USCS-MP3"):
        raise TunaError(f"Unrestricted {method[1:]} is not available in this build: MP3 runs on a closed-shell restricted reference.")
    if method in ("UCCD", "ULCCD"):
        raise TunaError(f"Unrestricted {method[1:]} is not available in this build: {method[1:]} runs on a closed-shell restricted reference.")
    if method in ("MP4", "MP4[SDTQ]", "MP4(SDTQ)"):
        raise TunaError(f"{method} is not available in this build: the triples of full fourth order need the (ov|vv) integrals and an "
                        "o^3 v^4 step this build does not have.  MP4(SDQ) is the fourth-order energy without them.")
    if method.startswith("UMP4"):
        raise TunaError(f"Unrestricted {method[1:]} is not available in this build: MP4 runs on a closed-shell restricted reference.")
    if method in ("CIS(D)", "CIS[D]", "UCIS(D)", "UCIS[D]"):
        raise TunaError(f"{method} is not available in this build: the perturbative doubles correction to CIS is not implemented.  CIS gives the "
                        "uncorrected states.  The keyword (D) on a CIS, TDHF, RPA or HF ... : TD line adds the doubles correction to the ROOT state.")
    if method in ("UCIS", "UTDHF", "URPA"):
        raise TunaError(f"Unrestricted {method[1:]} is not available in this build: {method[1:]} runs on a closed-shell restricted reference.")
    excited = method if method in ("CIS", "TDHF", "RPA") else None
    mp4 = {"MP4(SDQ)": "SDQ", "MP4[SDQ]": "SDQ", "MP4(DQ)": "DQ", "MP4[DQ]": "DQ"}.get(method)
    mp3 = method in ("MP3", "SCS-MP3")
    cc = method if method in ("CCD", "LCCD") else None       # coupled-cluster doubles; every other CC name stays unsupported
    if method not in ("HF", "RHF", "UHF", "MP2", "RMP2", "SCS-MP2", "MP3", "SCS-MP3", "CCD", "LCCD") and not mp4 and not excited and method not in dft_mod.FUNCTIONALS:
        raise TunaError(f"Electronic structure method \"{method}\" is not supported.")
    calc = interpret_keywords(params, Calculation(ctype, method if method in dft_mod.FUNCTIONALS else ("MP2" if "MP" in method else "HF"), basis))
    calc.coupled_cluster = cc
    if mp2_density_requested(calc):
        asked = " / ".join(k for k, on in (("RELAXED", calc.relaxed_density), ("UNRELAXED", calc.unrelaxed_density), ("NATORBS", calc.natural_orbitals)) if on)
        if unrestricted_mp2 or (calc.method == "MP2" and calc.multiplicity != 1):
            raise TunaError(f"{asked}: the unrestricted MP2 density is not built: the MP2 density and its natural orbitals are available on a "
                            "closed-shell restricted MP2 or SCS-MP2 line only.")
        if mp3 or mp4:
            raise TunaError(f"{asked}: the MP2 density on an {method} line is not built: the MP2 density and its natural orbitals are available on "
                            "a closed-shell restricted MP2 or SCS-MP2 line only.")
        if cc:
            raise TunaError(f"{asked}: the linearised coupled-cluster density is not built: the MP2 density and its natural orbitals are available on "
                            "a closed-shell restricted MP2 or SCS-MP2 line only.")
        if excited or calc.time_dependent:
            raise TunaError(f"{asked}: excited-state densities are not built: the MP2 density and its natural orbitals are available on a "
                            "closed-shell restricted MP2 or SCS-MP2 line only.")
        if calc.method != "MP2":
            raise TunaError(f"{asked}: densities and natural orbitals of a {method} line are not built: the MP2 density and its natural orbitals are "
                            "available on a closed-shell restricted MP2 or SCS-MP2 line only.")
        if calc.relaxed_density and calc.unrelaxed_density:
            raise TunaError("RELAXED and UNRELAXED ask for two different MP2 densities: give one of them.")
    if calc.time_dependent and not excited:                  # TD on an HF line: time-dependent Hartree-Fock (kernel:1175)
        if method in dft_mod.TD_AVAILABLE and not unrestricted_ks:
            # TD on a local-density Kohn-Sham line: TD-DFT, or its Tamm-Dancoff approximation with TDA (tuna_ci.py:2173-2201)
            if calc.do_perturbative_doubles:
                raise TunaError(f"The (D) keyword on a {method} ... : TD line: the perturbative doubles correction of a TD-DFT state (the "
                                "double-hybrid scaling of tuna_ci.py:1966) is not built.  (D) applies to a CIS, TDHF, RPA or HF ... : TD state.")
            excited = "TD-" + method                          # kernel:1299
        elif method not in ("HF", "RHF"):
            raise TunaError(f"The TD keyword is available on an HF or RHF line only in this build, and on the lines of the local-density "
                            f"functionals ({', '.join(dft_mod.TD_AVAILABLE)}): excited states of {'U' if unrestricted_ks else ''}{method} "
                            "(time-dependent DFT with a gradient-corrected or hybrid exchange-correlation kernel, unrestricted or correlated "
                            "references) are not implemented.")
        else:
            excited = "TD-HF"
    if excited:
        if calc.multiplicity != 1:
            raise TunaError(f"{excited} is available for a closed-shell restricted reference only in this build (ML 1).")
        if calc.dipole or calc.polarisability or calc.hyperpolarisability:
            raise TunaError("finite-field properties are available for Hartree-Fock energies in this build")
        if calc.calculate_no_singlets and calc.calculate_no_triplets:
            raise TunaError("There are no excited states to calculate!")                  # tuna_ci.py:2171
        calc.excited_state = excited
        calc.tamm_dancoff_approximation = calc.tamm_dancoff_approximation or excited == "CIS"      # tuna_ci.py:1314
    elif calc.do_perturbative_doubles:
        raise TunaError(f"The (D) keyword needs an excited-state method: the perturbative doubles correction applies to a CIS, TDHF, RPA or "
                        f"HF ... : TD state, not to {method}.")
    if cc and calc.multiplicity != 1:
        raise TunaError(f"{method} is available for a closed-shell restricted reference only in this build (ML 1).")
    if cc and (calc.dipole or calc.polarisability or calc.hyperpolarisability):
        raise TunaError("finite-field properties are available for Hartree-Fock energies in this build")
    calc.spin_component_scaling = method in ("SCS-MP2", "SCS-MP3")      # tuna_mp.py:872: "SCS" in the name scales the MP2 part too
    calc.mp3 = mp3
    calc.mp4 = mp4
    if mp4 and calc.multiplicity != 1:
        raise TunaError(f"{method} is available for a closed-shell restricted reference only in this build (ML 1).")
    if mp4 and (calc.dipole or calc.polarisability or calc.hyperpolarisability):
        raise TunaError("finite-field properties are available for Hartree-Fock energies in this build")
    if mp3 and calc.multiplicity != 1:
        raise TunaError(f"{method} is available for a closed-shell restricted reference only in this build (ML 1).")
    if mp3 and (calc.dipole or calc.polarisability or calc.hyperpolarisability):
        raise TunaError("finite-field properties are available for Hartree-Fock energies in this build")
    if method == "UHF":
        calc.reference = "UHF"
    if unrestricted_mp2:
        if calc.multiplicity == 1:
            # as for the Kohn-Sham singlet below: without the guess-orbital rotation the cycle stays on the restricted solution
            raise TunaError(f"Unrestricted {method} for a singlet needs the guess-orbital rotation, which this build does not have: "
                            f"use {method} for the restricted singlet, or ML n >= 2 for an open shell.")
        calc.reference = "UHF"
    if unrestricted_ks:
        if calc.multiplicity == 1:
            # the reference rotates the guess orbitals of an unrestricted singlet (tuna_guess.py:165-200, :396-398); without that rotation
            # the cycle would stay on the restricted solution and report it as unrestricted
            raise TunaError(f"Unrestricted {method} for a singlet needs the guess-orbital rotation, which this build does not have: "
                            f"use {method} for the restricted singlet, or ML n >= 2 for an open shell.")
        calc.reference = "UHF"
    if method in dft_mod.FUNCTIONALS:
        calc.functional = method
        if calc.stability_analysis:
            raise TunaError(f"STAB on a {method} line: the stability analysis of a Kohn-Sham solution (the orbital Hessian with the "
                            "exchange-correlation kernel) is not built.  STAB is available on Hartree-Fock references.")
    return calculate_energy(symbols, R, calc, engine, silent, log)
