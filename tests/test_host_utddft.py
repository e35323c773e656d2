"""CPU: the host side of unrestricted TD-DFT / TDA and of the Kohn-Sham stability analysis -- the two drivers run_unrestricted_tddft and
run_kohn_sham_stability on a stand-in engine that answers with the reference program's own numbers, their printed blocks against what
the reference prints (tests/golden/utddft_text.json) character for character, the routing in calculate_energy (a Calculation with a
functional of TD_AVAILABLE; both routes branch before run_excited_states / run_stability_analysis are called, which keep their
refusals), the functionals without a kernel, the input lines that stay refused, and the ctypes image of the new struct."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

import xc_kernel_reference as xk
from conftest import GOLD
from test_host_ucis import StabilityEngine, UnrestrictedEngine, keywords
from tuna_amd import _lib, dft, energy
from tuna_amd._lib import TunaError

KERNEL_LINES = [" Evaluating molecular orbitals on grid...    [Done]", " Evaluating exchange-correlation kernel...   [Done]",
                " Calculating matrix elements...              [Done]"]


@pytest.fixture(scope="module")
def texts():
    with open(os.path.join(GOLD, "utddft_text.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def utddft_golden(golden):
    return xk.split(golden("utddft_systems"))


class KohnShamEngine(UnrestrictedEngine, StabilityEngine):
    """tddft_uhf answers as the stand-in's cis_uhf does (the golden states of one run), stability_rks / _uks as its stability_rhf / _uhf;
    the Hartree-Fock entry points must not be reached"""

    def __init__(self, g=None, pre=None, vec=None, lowest=None):
        self.g, self.pre, self.vec, self.lowest, self.calls, self.extra = g, pre, vec, lowest, [], []

    def tddft_uhf(self, Ca, Cb, ea, eb, Pa, Pb, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0, **kw):
        self.extra.append(("tddft_uhf", Pa, Pb, kw.pop("hfx")))
        return UnrestrictedEngine.cis_uhf(self, Ca, Cb, ea, eb, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, **kw)

    def stability_rks(self, C, eps, P, n_occ, n_frozen=0, **kw):
        self.extra.append(("stability_rks", P, kw.pop("hfx")))
        return StabilityEngine.stability_rhf(self, C, eps, n_occ, n_frozen, **kw)

    def stability_uks(self, Ca, Cb, ea, eb, Pa, Pb, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0, **kw):
        self.extra.append(("stability_uks", Pa, Pb, kw.pop("hfx")))
        return StabilityEngine.stability_uhf(self, Ca, Cb, ea, eb, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, **kw)

    def cis_uhf(self, *a, **k):
        raise AssertionError("the Hartree-Fock routine was called on a Kohn-Sham reference")
    stability_rhf = stability_uhf = cis_uhf


def nh_atoms():
    return [types.SimpleNamespace(symbol=s, charge=z, origin=np.array([0.0, 0.0, k * 1.036 / 0.5291772105])) for k, (s, z) in enumerate((("N", 7), ("H", 1)))]


def objects(g):
    from tuna_amd import molecule as mol
    N = len(g["eps_alpha"])
    atoms = mol.make_atoms(["N", "H"], mol.angstrom_to_bohr(1.036))
    molecule = types.SimpleNamespace(n_basis=N, n_alpha=int(g["n_alpha"]), n_beta=int(g["n_beta"]), n_electrons=int(g["n_alpha"]) + int(g["n_beta"]), atoms=atoms)
    out = types.SimpleNamespace(molecular_orbitals_alpha=g["C_alpha"], molecular_orbitals_beta=g["C_beta"], epsilons_alpha=g["eps_alpha"],
                                epsilons_beta=g["eps_beta"], P_alpha=g["P_alpha"], P_beta=g["P_beta"], energy=float(g["E_SCF"]), timings={})
    return molecule, types.SimpleNamespace(D=g["dip"]), out


def ks_calc(text, functional, reference="UHF", excited=None):
    calc = keywords(text)
    calc.reference, calc.functional, calc.HFX_prop = reference, functional, 0.0
    if excited:
        calc.excited_state = excited
    return calc


def test_unrestricted_tddft_blocks_are_the_reference_s(texts, utddft_golden):
    """One TD and one TD TDA run of NH / STO-3G HFS: from the first line of the kernel build to the end of the spectrum table, character
    for character, with the vectors the reference printed from; out.energy = E_SCF + w_root; the densities and HFX reach the engine."""
    blocks = [t for t in texts if t["kind"] == "excited"]
    assert {t["method"] for t in blocks} == {"TDDFT", "TDA"}
    for t in blocks:
        g = utddft_golden[t["system"]]
        for spin in "ab":
            assert [s for s in t["labels"] if s.endswith(spin)] == [f"{k + 1}{spin}" for k in range(len(g["eps_alpha"]))]
        for root in (1, 3):
            calc = ks_calc(f"NSTATES {t['n_states']} ROOT {root}" + (" TDA" if t["method"] == "TDA" else ""), t["functional"], excited="TD-" + t["functional"])
            molecule, integrals, out = objects(g)
            eng, log = KohnShamEngine(g, t["prefix"], t["vectors"]), []
            energy.run_unrestricted_tddft(calc, molecule, integrals, out, eng, silent=False, log=log.append)
            na, nb, nfa, nfb, kw, dip = eng.calls[0]
            assert (na, nb, nfa, nfb) == (molecule.n_alpha, molecule.n_beta, 0, 0) and dip is integrals.D
            assert kw == {"method": t["method"], "n_keep": max(t["n_states"], root)}
            assert eng.extra == [("tddft_uhf", out.P_alpha, out.P_beta, 0.0)]
            want = g[t["prefix"] + "energies"]
            assert abs(out.energy - (float(g["E_SCF"]) + want[root - 1])) < 1e-8 and out.excited["E_transition"] == want[root - 1]
            text = "\n".join(log).split("\n")
            start = text.index(KERNEL_LINES[0])
            end = max(n for n, s in enumerate(text) if s.startswith(" ~~~~"))
            ref = t["text"].strip("\n").split("\n")
            assert text[start:end + 1] == ref, "\n".join(a + "   |   " + b for a, b in zip(text[start:end + 1], ref) if a != b)
            joined = "\n".join(text)
            assert "Singlet" not in joined and "states will be calculated" not in joined
            assert f" Excitation energy from {'TD-' + t['functional'] + ':':<11} {want[root - 1]:15.10f}" in joined
    # refusals of this route
    g = utddft_golden[blocks[0]["system"]]
    for functional, reference, match in (("B3LYP", "UHF", "not yet available"), ("BLYP", "UHF", "not yet available"), (None, "UHF", "not yet available"),
                                         ("HFS", "RHF", "unrestricted")):
        calc = ks_calc("", functional, reference, excited="TD")
        with pytest.raises(TunaError, match=match):
            energy.run_unrestricted_tddft(calc, *objects(g), KohnShamEngine(g, blocks[0]["prefix"], blocks[0]["vectors"]))
    calc = ks_calc("", "HFS", excited="TD-HFS")
    calc.do_perturbative_doubles = True
    with pytest.raises(TunaError, match=r"\(D\)"):
        energy.run_unrestricted_tddft(calc, *objects(g), KohnShamEngine(g, blocks[0]["prefix"], blocks[0]["vectors"]))


def test_kohn_sham_stability_blocks_are_the_reference_s(texts):
    blocks = [t for t in texts if t["kind"] == "stability"]
    assert {t["reference"] for t in blocks} == {"RHF", "UHF"}
    N = 10
    molecule = types.SimpleNamespace(n_basis=N, n_doubly_occ=5, n_alpha=5, n_beta=3, n_electrons=8, atoms=nh_atoms())
    P = np.full((N, N), 0.5)
    out = types.SimpleNamespace(molecular_orbitals=np.eye(N), epsilons=np.arange(N, dtype=float), molecular_orbitals_alpha=np.eye(N),
                                molecular_orbitals_beta=np.eye(N), epsilons_alpha=np.arange(N, dtype=float), epsilons_beta=np.arange(N, dtype=float),
                                P=P, P_alpha=P / 2, P_beta=P / 4, energy=-1.0, timings={})
    for t in blocks:
        calc = ks_calc("STAB", t["functional"], t["reference"])
        eng, log = KohnShamEngine(lowest=t["lowest"]), []
        energy.run_kohn_sham_stability(calc, molecule, out, eng, silent=False, log=log.append)
        if t["reference"] == "UHF":
            assert eng.calls == [("uhf", 5, 3, 0, 0)] and eng.extra == [("stability_uks", out.P_alpha, out.P_beta, 0.0)]
        else:
            assert eng.calls == [("rhf", 5, 0)] and eng.extra == [("stability_rks", out.P, 0.0)]
        text = "\n".join(log).split("\n")
        k = next(n for n, s in enumerate(text) if "Stability Analysis" in s)
        assert [s for s in text[:k - 1] if s] == KERNEL_LINES                                  # the kernel build's three lines come first
        assert text[k - 1:] == t["text"].strip("\n").split("\n")
        st = out.stability
        assert st["threshold"] == -1e-5 and st["stable"] and out.energy == -1.0 and st["reference"] == t["reference"]
    # an unstable solution is a result; freeze_core reaches the engine; silent prints nothing
    calc = ks_calc("STAB", "SVWN", "UHF")
    calc.freeze_core = True
    eng, log = KohnShamEngine(lowest=[-0.3]), []
    energy.run_kohn_sham_stability(calc, molecule, out, eng, silent=True, log=log.append)
    assert not log and eng.calls == [("uhf", 5, 3, 1, 1)] and out.stability["unstable_unrestricted"] and not out.stability["stable"]
    for functional in ("B3LYP", "BLYP", "PBE", None):
        with pytest.raises(TunaError, match="not yet available"):
            energy.run_kohn_sham_stability(ks_calc("STAB", functional, "RHF"), molecule, out, KohnShamEngine(lowest=[0.1, 0.1]))


def test_routing_in_calculate_energy(monkeypatch):
    """A Calculation with a functional of TD_AVAILABLE: STAB goes to run_kohn_sham_stability, excited states of a UHF reference to
    run_unrestricted_tddft -- run_stability_analysis and run_excited_states are not called.  Every other Calculation takes the routes
    it took, refusals included."""
    order = []
    out = types.SimpleNamespace(energy=-1.0, timings={}, molecular_orbitals=None, epsilons=None)
    molecule = types.SimpleNamespace(atoms=[], n_doubly_occ=1, n_alpha=1, n_beta=1)
    monkeypatch.setattr(energy, "build_molecule_and_integrals", lambda *a, **k: (molecule, types.SimpleNamespace(), None, None, {}))
    monkeypatch.setattr(energy.mol, "nuclear_repulsion", lambda atoms: 0.0)
    monkeypatch.setattr(energy, "run_self_consistent_field_cycle", lambda *a, **k: order.append("scf") or out)
    for name in ("run_stability_analysis", "run_kohn_sham_stability", "run_excited_states", "run_unrestricted_tddft"):
        monkeypatch.setattr(energy, name, lambda *a, _n=name, **k: order.append(_n))

    def route(functional, reference, stab, excited):
        order.clear()
        calc = keywords("STAB" if stab else "")
        calc.functional, calc.reference, calc.excited_state = functional, reference, excited
        energy.calculate_energy(["H", "H"], 1.4, calc, engine=object())
        return order[1:]
    assert set(dft.TD_AVAILABLE) >= {"HFS", "SVWN", "LDA", "LSDA", "SVWN5", "SVWN3"}
    for f in dft.TD_AVAILABLE:
        assert route(f, "UHF", True, "TD-" + f) == ["run_kohn_sham_stability", "run_unrestricted_tddft"]
        assert route(f, "RHF", True, "TD-" + f) == ["run_kohn_sham_stability", "run_excited_states"]
        assert route(f, "UHF", False, None) == []
    for f in ("B3LYP", "BLYP", None):
        assert route(f, "UHF", True, "TD") == ["run_stability_analysis", "run_excited_states"]
        assert route(f, "RHF", True, "CIS") == ["run_stability_analysis", "run_excited_states"]


def test_existing_refusals_stay(utddft_golden):
    """run_excited_states and run_stability_analysis keep raising for a Kohn-Sham reference, and the input lines stay refused"""
    g = utddft_golden["nh_hfs_sto3g"]
    calc = ks_calc("", "HFS", excited="TD-HFS")
    with pytest.raises(TunaError, match="Unrestricted time-dependent DFT is not built"):
        energy.run_excited_states(calc, *objects(g), KohnShamEngine(g, "TDA_fc0_", "text_1_"))
    with pytest.raises(TunaError, match="exchange-correlation kernel"):
        energy.run_stability_analysis(ks_calc("STAB", "SVWN", "RHF"), *objects(g)[::2], KohnShamEngine(lowest=[0.1, 0.1]))
    for line in ("SPE : C O 1.128 : LDA 6-31G : STAB", "SPE : C O 1.128 : SVWN 6-31G : TD STAB", "SPE : O O 1.2075 : ULDA STO-3G : TD ML 3",
                 "SPE : O O 1.2075 : LDA STO-3G : TD ML 3", "SPE : O O 1.2075 : UB3LYP STO-3G : ML 3 STAB"):
        with pytest.raises(TunaError):
            energy.run(line, engine=object())


def test_struct_image_and_exports():
    assert ctypes.sizeof(_lib.UtddftOpts) == 16 and _lib.UtddftOpts.hfx.offset == 8
    for name in ("tf_xc_kernel_spin_plan", "tf_xc_kernel_spin_probe", "tf_xc_kernel_uhf", "tf_tddft_uhf", "tf_stability_rks", "tf_stability_uks"):
        assert name in _lib.EXPORTS
    from tuna_amd.engine import Engine
    for name in ("xc_kernel_spin_plan", "xc_kernel_spin_probe", "xc_kernel_uhf", "tddft_uhf", "stability_rks", "stability_uks"):
        assert callable(getattr(Engine, name))
