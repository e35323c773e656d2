"""CPU: the host side of the STAB keyword and of the unrestricted excited states -- the keyword, its routing on Hartree-Fock, UHF and
correlated lines and its refusal on a Kohn-Sham line, the printed stability block and the unrestricted contribution / spectrum blocks
against what the reference prints (tests/golden/stability_text.json; a stand-in engine answers with the reference program's own
numbers), the Calculation route to tf_cis_uhf with ROOT, NSTATES, EXTHRESH, TDA and freeze_core, the input-line names that stay refused,
and the ctypes image of the new structs."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

from conftest import GOLD
from test_cis_reference import split
from test_gpu_cis import same_table
from tuna_amd import _lib, energy
from tuna_amd._lib import TunaError


def keywords(text):
    return energy.interpret_keywords(text.split(), energy.Calculation())


def routed(line, monkeypatch):
    seen = {}
    monkeypatch.setattr(energy, "calculate_energy", lambda symbols, R, calc, engine, silent, log: seen.setdefault("calc", calc))
    energy.run(line)
    return seen["calc"]


@pytest.fixture(scope="module")
def texts():
    with open(os.path.join(GOLD, "stability_text.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ucis_golden(golden):
    return split(golden("ucis_systems"))


def test_stab_keyword_and_routing(monkeypatch):
    assert not keywords("").stability_analysis and not keywords("").freeze_core and keywords("TIGHT STAB").stability_analysis
    for line, method, reference in (("SPE : H H 2.0 : HF STO-3G : STAB", "HF", "RHF"), ("SPE : C O 1.128 : MP2 6-31G : STAB", "MP2", "RHF"),
                                    ("SPE : C O 1.128 : CCD 6-31G : STAB", "HF", "RHF"), ("SPE : C O 1.128 : CIS 6-31G : STAB", "HF", "RHF"),
                                    ("SPE : O O 1.2075 : UHF STO-3G : ML 3 STAB", "HF", "UHF")):
        c = routed(line, monkeypatch)
        assert c.stability_analysis and c.method == method and c.functional is None and (c.reference == reference or c.multiplicity == 3)
    assert not routed("SPE : C O 1.128 : HF 6-31G", monkeypatch).stability_analysis
    for line in ("SPE : C O 1.128 : B3LYP 6-31G : STAB", "SPE : O O 1.2075 : UB3LYP STO-3G : ML 3 STAB", "SPE : C O 1.128 : LDA 6-31G : STAB"):
        with pytest.raises(TunaError, match="exchange-correlation kernel"):
            routed(line, monkeypatch)


@pytest.mark.parametrize("line", ["SPE : N N 1.0977 : UCIS STO-3G", "SPE : N N 1.0977 : UTDHF STO-3G", "SPE : N N 1.0977 : URPA STO-3G",
                                  "SPE : O O 1.2075 : CIS STO-3G : ML 3", "SPE : O O 1.2075 : HF STO-3G : TD ML 3", "SPE : O O 1.2075 : UHF STO-3G : TD ML 3"])
def test_input_line_names_stay_refused(monkeypatch, line):
    with pytest.raises(TunaError):
        routed(line, monkeypatch)


class StabilityEngine:
    def __init__(self, lowest):
        self.lowest, self.calls = lowest, []

    def stability_rhf(self, C, eps, n_occ, n_frozen=0, **kw):
        self.calls.append(("rhf", n_occ, n_frozen))
        return {"dim": n_occ * (len(eps) - n_occ), "lowest_singlet": self.lowest[0], "lowest_triplet": self.lowest[1], "source_singlet": "minus",
                "source_triplet": "plus_triplet", "seconds": [0.0] * 4}

    def stability_uhf(self, Ca, Cb, ea, eb, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0, **kw):
        self.calls.append(("uhf", n_alpha, n_beta, n_frozen_alpha, n_frozen_beta))
        return {"dim": 30, "dim_alpha": 9, "lowest": self.lowest[0], "source": "plus", "seconds": [0.0] * 4}


def atoms_of(charges):
    """O2 at 1.2075 angstrom, or one atom"""
    return [types.SimpleNamespace(symbol={8: "O", 3: "LI"}[z], charge=z, origin=np.array([0.0, 0.0, k * 1.2075 / 0.5291772105])) for k, z in enumerate(charges)]


def test_stability_block_is_the_reference_s(texts):
    blocks = [t for t in texts if t["kind"] == "stability"]
    assert {t["reference"] for t in blocks} == {"RHF", "UHF"} and len(blocks) == 3
    for t in blocks:
        calc = keywords("STAB")
        calc.reference = t["reference"]
        N = 10
        molecule = types.SimpleNamespace(n_basis=N, n_doubly_occ=7, n_alpha=9, n_beta=7, n_electrons=16, atoms=atoms_of([8, 8]))
        out = types.SimpleNamespace(molecular_orbitals=np.eye(N), epsilons=np.arange(N, dtype=float), molecular_orbitals_alpha=np.eye(N),
                                    molecular_orbitals_beta=np.eye(N), epsilons_alpha=np.arange(N, dtype=float), epsilons_beta=np.arange(N, dtype=float),
                                    energy=-1.0, timings={})
        eng, log = StabilityEngine(t["lowest"]), []
        energy.run_stability_analysis(calc, molecule, out, eng, silent=False, log=log.append)
        assert eng.calls == ([("uhf", 9, 7, 0, 0)] if t["reference"] == "UHF" else [("rhf", 7, 0)])
        same_table("\n".join(log).strip("\n").split("\n"), t["text"].strip("\n").split("\n"))
        st = out.stability
        assert st["threshold"] == -1e-5 and st["stable"] == all(x > -1e-5 for x in t["lowest"]) and out.energy == -1.0
        if t["reference"] == "RHF":
            assert (st["lowest_singlet"], st["lowest_triplet"]) == tuple(t["lowest"]) and st["unstable_unrestricted"] == (t["lowest"][1] <= -1e-5)
        # silent: the same result, nothing printed; freeze_core: the core orbitals leave the window of either spin
        calc.freeze_core = True
        eng2, log2 = StabilityEngine(t["lowest"]), []
        energy.run_stability_analysis(calc, molecule, out, eng2, silent=True, log=log2.append)
        assert not log2 and eng2.calls == ([("uhf", 9, 7, 2, 2)] if t["reference"] == "UHF" else [("rhf", 7, 2)]) and out.stability["n_frozen"] == 2
    # the three verdict sentences
    seen = set()
    for lowest, reference in (([0.3, 0.1], "RHF"), ([-0.2, 0.1], "RHF"), ([0.2, -0.1], "RHF"), ([-0.2, -0.1], "RHF"), ([0.2], "UHF"), ([-0.2], "UHF")):
        calc = keywords("STAB")
        calc.reference = reference
        log = []
        energy.run_stability_analysis(calc, molecule, out, StabilityEngine(lowest), silent=False, log=log.append)
        text = "\n".join(log)
        verdicts = tuple(s in text for s in ("unstable wrt. restricted rotations.", "unstable wrt. unrestricted rotations.", "solution is stable!"))
        assert verdicts == (reference == "RHF" and lowest[0] <= -1e-5, lowest[-1] <= -1e-5, all(x > -1e-5 for x in lowest))
        seen.add(verdicts)
    assert len(seen) == 4
    calc = keywords("STAB")
    calc.functional = "B3LYP"
    with pytest.raises(TunaError, match="exchange-correlation kernel"):
        energy.run_stability_analysis(calc, molecule, out, StabilityEngine([0.1, 0.1]))


def test_stab_runs_after_the_scf_and_before_the_post_scf_stage(monkeypatch):
    order = []
    out = types.SimpleNamespace(energy=-1.0, timings={}, molecular_orbitals=None, epsilons=None)
    molecule = types.SimpleNamespace(atoms=[], n_doubly_occ=1, n_alpha=1, n_beta=1)
    monkeypatch.setattr(energy, "build_molecule_and_integrals", lambda *a, **k: (molecule, types.SimpleNamespace(), None, None, {}))
    monkeypatch.setattr(energy.mol, "nuclear_repulsion", lambda atoms: 0.0)
    monkeypatch.setattr(energy, "run_self_consistent_field_cycle", lambda *a, **k: order.append("scf") or out)
    monkeypatch.setattr(energy, "run_stability_analysis", lambda *a, **k: order.append("stab"))
    monkeypatch.setattr(energy, "run_coupled_cluster_doubles", lambda *a, **k: order.append("ccd"))
    monkeypatch.setattr(energy, "run_excited_states", lambda *a, **k: order.append("excited"))
    calc = keywords("STAB")
    calc.coupled_cluster, calc.excited_state = "CCD", "CIS"
    energy.calculate_energy(["H", "H"], 1.4, calc, engine=object())
    assert order == ["scf", "stab", "ccd", "excited"]
    order.clear()
    energy.calculate_energy(["H", "H"], 1.4, keywords(""), engine=object())
    assert order == ["scf"]


class UnrestrictedEngine:
    """Answers cis_uhf with the golden states of one run: all energies, |mu| along z and f, and the vectors the reference printed from."""

    def __init__(self, g, pre, vec):
        self.g, self.pre, self.vec, self.calls = g, pre, vec, []

    def cis_uhf(self, Ca, Cb, ea, eb, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0, **kw):
        self.calls.append((n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, {k: v for k, v in kw.items() if k != "dip"}, kw.get("dip")))
        g, pre = self.g, self.pre
        e = g[pre + "energies"]
        N, dim = len(ea), len(e)
        tdm = np.zeros((dim, 3))
        tdm[:, 2] = g[pre + "tdm"]
        nk = min(kw["n_keep"], dim)
        X, Y = np.zeros((nk, dim)), np.zeros((nk, dim))
        have = min(nk, len(g[self.vec + "X"]))
        X[:have], Y[:have] = g[self.vec + "X"][:have], g[self.vec + "Y"][:have]
        return {"dim": dim, "dim_alpha": (n_alpha - n_frozen_alpha) * (N - n_alpha), "E": e, "X": X, "Y": Y, "tdm": tdm, "osc": g[pre + "osc"], "seconds": [0.0] * 4}


def unrestricted_objects(g, charges):
    N = len(g["eps_alpha"])
    molecule = types.SimpleNamespace(n_basis=N, n_alpha=int(g["n_alpha"]), n_beta=int(g["n_beta"]), n_electrons=int(g["n_alpha"]) + int(g["n_beta"]),
                                     atoms=atoms_of(charges))
    out = types.SimpleNamespace(molecular_orbitals_alpha=g["C_alpha"], molecular_orbitals_beta=g["C_beta"], epsilons_alpha=g["eps_alpha"],
                                epsilons_beta=g["eps_beta"], energy=float(g["E_UHF"]), timings={})
    return molecule, types.SimpleNamespace(D=g["dip"]), out


def test_unrestricted_blocks_are_the_reference_s(texts, ucis_golden):
    """The contribution and spectrum blocks, spin-orbital labels such as "7b -> 8b" included, from the vectors the reference printed from;
    out.energy = E_SCF + w_root within 1e-8; the way in is the Calculation, through run_excited_states."""
    blocks = [t for t in texts if t["kind"] == "excited"]
    assert {t["method"] for t in blocks} == {"CIS", "TDHF"}
    for t in blocks:
        g = ucis_golden[t["system"]]
        charges = [8, 8] if t["system"].startswith("o2") else [3]
        # the reference's labels in its combined energy order are, spin by spin, the spin's own numbering
        for spin in "ab":
            assert [s for s in t["labels"] if s.endswith(spin)] == [f"{k + 1}{spin}" for k in range(len(g["eps_alpha"]))]
        for root in (1, 3):
            calc = keywords(f"NSTATES {t['n_states']} ROOT {root}")
            calc.reference, calc.excited_state, calc.tamm_dancoff_approximation = "UHF", t["method"], t["method"] == "CIS"
            molecule, integrals, out = unrestricted_objects(g, charges)
            eng, log = UnrestrictedEngine(g, t["prefix"], t["vectors"]), []
            energy.run_excited_states(calc, molecule, integrals, out, eng, silent=False, log=log.append)
            na, nb, nfa, nfb, kw, dip = eng.calls[0]
            assert (na, nb, nfa, nfb) == (molecule.n_alpha, molecule.n_beta, 0, 0) and dip is integrals.D
            assert kw == {"method": t["method"], "n_keep": max(t["n_states"], root)}
            want = g[t["prefix"] + "energies"]
            assert abs(out.energy - (float(g["E_UHF"]) + want[root - 1])) < 1e-8 and out.excited["E_transition"] == want[root - 1]
            assert out.excited["X_alpha"].shape == (na, len(g["eps_alpha"]) - na) and out.excited["Y_beta"].shape == (nb, len(g["eps_beta"]) - nb)
            text = "\n".join(log).split("\n")
            start = next(n for n, s in enumerate(text) if s.startswith("  Printing excited state information"))
            end = max(n for n, s in enumerate(text) if s.startswith(" ~~~~"))
            ref = t["text"].strip("\n").split("\n")
            same_table(text[start:end + 1], ref)
            joined = "\n".join(text)
            assert " - S " not in joined and " - T " not in joined and "Singlet" not in joined and "states will be calculated" not in joined
            assert f" Excitation energy from {t['method'] + ':':<11} {want[root - 1]:15.10f}" in joined
    # EXTHRESH, freeze_core and the refusals of this route
    t = blocks[0]
    g = ucis_golden[t["system"]]
    calc = keywords("NSTATES 2 EXTHRESH 50")
    calc.reference, calc.excited_state, calc.tamm_dancoff_approximation, calc.freeze_core = "UHF", "CIS", True, True
    molecule, integrals, out = unrestricted_objects(g, [8, 8])
    eng, log = UnrestrictedEngine(g, t["prefix"], t["vectors"]), []
    with pytest.raises(Exception):
        # the stand-in's vectors belong to the all-electron windows: the frozen windows must reach the engine before anything is printed
        energy.run_excited_states(calc, molecule, integrals, out, eng, silent=False, log=log.append)
    assert eng.calls[0][:4] == (9, 7, 2, 2)
    calc.freeze_core = False
    molecule, integrals, out = unrestricted_objects(g, [8, 8])
    log = []
    energy.run_excited_states(calc, molecule, integrals, out, UnrestrictedEngine(g, t["prefix"], t["vectors"]), silent=False, log=log.append)
    assert all(float(s.split()[-2]) > 50 for s in "\n".join(log).split("\n") if "->" in s) and "Only printing contributions larger than 50.0 %." in "\n".join(log)
    calc.root = 400
    with pytest.raises(TunaError, match=r"Specified root \(400\) does not exist!"):
        energy.run_excited_states(calc, *unrestricted_objects(g, [8, 8]), UnrestrictedEngine(g, t["prefix"], t["vectors"]))
    calc.root, calc.do_perturbative_doubles = 1, True
    with pytest.raises(TunaError, match=r"\(D\)"):
        energy.run_excited_states(calc, *unrestricted_objects(g, [8, 8]), UnrestrictedEngine(g, t["prefix"], t["vectors"]))


def test_struct_images():
    assert ctypes.sizeof(_lib.UcisOpts) == 8 and ctypes.sizeof(_lib.UcisResult) == 8 + 7 * 8 + 32
    assert _lib.UcisResult.e.offset == 8 and _lib.UcisResult.seconds.offset == 64
    assert ctypes.sizeof(_lib.StabilityResult) == 24 + 16 + 16 + 32 and _lib.StabilityResult.lowest.offset == 24 and _lib.StabilityResult.spectra.offset == 40
    for name in ("tf_cis_uhf", "tf_stability_rhf", "tf_stability_uhf"):
        assert name in _lib.EXPORTS
