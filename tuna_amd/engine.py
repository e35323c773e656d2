"""Engine -- one context of libtunafock per process/GPU: basis set-up, device-resident ERI tensor,
Fock builds and the native RHF cycle.  Thin: every numerical step happens in the HIP library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import ScfOpts, ScfResult, ScfUhfResult, TunaError, f64, i32, ptr
from .molecule import AOList

# SCF convergence thresholds (tuna_util.py:109-116)
SCF_CONVERGENCE = {
    "loose": {"delta_E": 0.000001, "max_DP": 0.00001, "RMS_DP": 0.000001, "commutator": 0.0001, "name": "loose"},
    "medium": {"delta_E": 0.0000001, "max_DP": 0.000001, "RMS_DP": 0.0000001, "commutator": 0.00001, "name": "medium"},
    "tight": {"delta_E": 0.000000001, "max_DP": 0.00000001, "RMS_DP": 0.000000001, "commutator": 0.0000001, "name": "tight"},
    "extreme": {"delta_E": 0.00000000001, "max_DP": 0.0000000001, "RMS_DP": 0.00000000001, "commutator": 0.000000001,
                "name": "extreme"},
}


class Engine:
    def __init__(self, device: int = 0, rank: int = 0, world: int = 1):
        self._L = _lib.lib()
        self._ctx = self._L.tf_create(int(device), int(rank), int(world))
        if not self._ctx:
            raise TunaError(self._L.tf_last_error(None).decode(), -2)
        self.device, self.rank, self.world = device, rank, world
        self.aos: AOList | None = None
        self.n_cart = self.n_sph = self.n_shell = 0
        self.N = 0
        self.spherical = True

    # ---- plumbing --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._L.tf_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != 0:
            raise TunaError(self._L.tf_last_error(self._ctx).decode(), rc)

    # ---- basis -----------------------------------------------------------------------------
    def set_basis(self, aos: AOList):
        self.aos = aos
        self._keep = (f64(aos.origin), i32(aos.lmn), i32(aos.prim_off), f64(aos.exps), f64(aos.coefs))
        o, l, p, e, c = self._keep
        self._check(self._L.tf_set_basis(self._ctx, aos.n, ptr(o), ptr(l), ptr(p), ptr(e), ptr(c)))
        a, b, s = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.tf_dims(self._ctx, a, b, s))
        self.n_cart, self.n_sph, self.n_shell = a.value, b.value, s.value
        return self

    def norms(self):
        norm = np.zeros_like(self.aos.exps)
        coef = np.zeros_like(self.aos.exps)
        self._check(self._L.tf_get_norms(self._ctx, ptr(norm), ptr(coef)))
        return norm, coef

    def sph_matrix(self) -> np.ndarray:
        U = np.zeros((self.n_sph, self.n_cart))
        self._check(self._L.tf_get_sph_matrix(self._ctx, ptr(U)))
        return U

    # ---- one-electron ------------------------------------------------------------------------
    def one_electron(self, atom_xyz, atom_charge, dipole_origin, spherical: bool = True):
        n = self.n_sph if spherical else self.n_cart
        xyz, chg, org = f64(np.asarray(atom_xyz).reshape(-1, 3)), f64(atom_charge), f64(dipole_origin)
        S, T, V = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
        D, Q = np.zeros((3, n, n)), np.zeros((3, n, n))
        self._check(self._L.tf_one_electron(self._ctx, len(chg), ptr(xyz), ptr(chg), ptr(org), int(spherical),
                                            ptr(S), ptr(T), ptr(V), ptr(D), ptr(Q)))
        return S, T, V, D, Q

    def cross_overlap(self, other: AOList) -> np.ndarray:
        S = np.zeros((self.n_cart, other.n))
        o, l, p, e, c = f64(other.origin), i32(other.lmn), i32(other.prim_off), f64(other.exps), f64(other.coefs)
        self._check(self._L.tf_cross_overlap(self._ctx, other.n, ptr(o), ptr(l), ptr(p), ptr(e), ptr(c), ptr(S)))
        return S

    # ---- two-electron ------------------------------------------------------------------------
    LAYOUTS = {"auto": -1, "rows": 0, "packed": 1, "tiles": 2}

    def build_eri(self, spherical: bool = True, layout: str | None = None):
        """layout: "packed" (8-fold unique values, the default where the J/K kernel covers N), "rows" ((i >= j) x full [k][l])
        or None / "auto"."""
        if layout is not None:
            self._check(self._L.tf_set_eri_layout(self._ctx, self.LAYOUTS[layout]))
        self._check(self._L.tf_build_eri(self._ctx, int(spherical)))
        self.spherical = spherical
        self.N = self.n_sph if spherical else self.n_cart
        return self

    def eri_storage(self) -> dict:
        b, r = C.c_int64(), C.c_int64()
        n, ld = C.c_int32(), C.c_int32()
        self._check(self._L.tf_eri_storage(self._ctx, b, r, n, ld))
        return {"bytes": b.value, "rows": r.value, "N": n.value, "ld": ld.value,
                "layout": {2: "tiles", 1: "packed"}.get(self._L.tf_eri_layout(self._ctx), "rows")}

    def eri_timings(self) -> dict:
        t = np.zeros(4)
        self._check(self._L.tf_eri_timings(self._ctx, ptr(t)))
        c = np.zeros(3, dtype=np.int64)
        self._check(self._L.tf_eri_counts(self._ctx, ptr(c)))
        f = np.zeros(1)
        self._check(self._L.tf_eri_flops(self._ctx, ptr(f)))
        return {"total_s": t[0], "cart_kernel_s": t[1], "ket_transform_s": t[2], "bra_transform_s": t[3],
                "shell_quartets": int(c[0]), "primitive_shell_quartets": int(c[1]), "component_quartets": int(c[2]),
                "nominal_flops": float(f[0])}

    # counters of tf_eri_build_stats, in the order of the TF_ERI_STAT_* list of tunafock.h
    ERI_BUILD_STATS = ("slabs", "launches", "team16", "team64", "team256", "team_flat", "teamc", "cfact_uncontracted", "cfact_contracted",
                       "cfact_gtab", "cfact_ket_families", "cfact_both_families", "cfact_bra_families", "component_lane", "multi", "fact",
                       "class_staged", "class_unstaged")

    def eri_build_stats(self) -> dict:
        """Launch structure of the last build_eri: slabs and launches per kernel family (tunafock.h: tf_eri_build_stats)."""
        out = (C.c_int64 * len(self.ERI_BUILD_STATS))()
        self._check(self._L.tf_eri_build_stats(self._ctx, out, len(out)))
        return dict(zip(self.ERI_BUILD_STATS, (int(v) for v in out)))

    def copy_eri(self, out: np.ndarray | None = None) -> np.ndarray:
        N = self.N
        if out is None:
            out = np.empty((N, N, N, N))
        assert out.flags.c_contiguous and out.dtype == np.float64 and out.size == N ** 4
        self._check(self._L.tf_copy_eri(self._ctx, ptr(out)))
        return out

    def sample_eri(self, idx) -> np.ndarray:
        idx = i32(idx).reshape(-1, 4)
        out = np.zeros(len(idx))
        self._check(self._L.tf_sample_eri(self._ctx, len(idx), ptr(idx), ptr(out)))
        return out

    def eri_element(self, aos4: AOList) -> float:
        v = C.c_double()
        o, l, p, e, c = f64(aos4.origin), i32(aos4.lmn), i32(aos4.prim_off), f64(aos4.exps), f64(aos4.coefs)
        self._check(self._L.tf_eri_element(self._ctx, ptr(o), ptr(l), ptr(p), ptr(e), ptr(c), C.byref(v)))
        return v.value

    # ---- Fock build --------------------------------------------------------------------------
    def fock_jk(self, P: np.ndarray):
        """J, K for one [N,N] or several [n,N,N] densities (host buffers).  Partial sums when world > 1, unless a communicator is
        attached (comm_init): then the library has summed them over the ranks."""
        P = f64(P)
        if self._L.tf_eri_layout(self._ctx) >= 0 and (P.ndim not in (2, 3) or P.shape[-1] != self.N or P.shape[-2] != self.N):   # (no tensor yet: the library reports that)
            raise ValueError(f"fock_jk: densities must be [{self.N},{self.N}] or [n,{self.N},{self.N}], got {P.shape}")
        nd = 1 if P.ndim == 2 else P.shape[0]
        J, K = np.zeros_like(P), np.zeros_like(P)
        self._check(self._L.tf_fock_jk(self._ctx, nd, ptr(P), ptr(J), ptr(K)))
        return J, K

    def fock_jk_device(self, dP: int, dJ: int, dK: int, n_dens: int = 1, stream: int = 0):
        """Device-pointer variant (integers from tensor.data_ptr()); asynchronous on `stream`."""
        self._check(self._L.tf_fock_jk_device(self._ctx, n_dens, C.c_void_p(dP), C.c_void_p(dJ), C.c_void_p(dK),
                                              C.c_void_p(stream)))

    def jk_profile(self, enable: bool):
        self._check(self._L.tf_jk_profile(self._ctx, int(enable)))

    def jk_profile_read(self):
        """(seconds summed over launches, launches) of the row kernel since profiling was enabled."""
        s, n = C.c_double(), C.c_int64()
        self._check(self._L.tf_jk_profile_read(self._ctx, C.byref(s), C.byref(n)))
        return s.value, n.value

    # ---- SCF -----------------------------------------------------------------------------------
    def orthogonaliser(self, S: np.ndarray):
        S = f64(S)
        n = S.shape[0]
        X, Si = np.zeros((n, n)), np.zeros((n, n))
        sm = C.c_double()
        self._check(self._L.tf_orthogonaliser(self._ctx, n, ptr(S), ptr(X), ptr(Si), C.byref(sm)))
        return X, sm.value, Si

    # ---- Kohn-Sham exchange-correlation ------------------------------------------------------------
    def dft_setup(self, points, weights, functional: str | None, x_alpha: float = 2 / 3) -> dict:
        """Puts the grid on the device, evaluates the AOs on it and selects the functional (tuna_amd.dft.FUNCTIONALS; None: no functional).
        While set, scf_rhf runs restricted Kohn-Sham; returns {"hfx": HFX_prop, ...} to pass on."""
        from . import dft
        if functional is None:                                # the null functional: exact exchange alone (tddft_rhf is then TDHF / CIS)
            name, (xn, cn, dfx, hfx, dfc) = "NONE", (None, None, 0.0, 1.0, 0.0)
        else:
            name = functional.upper()
            if name not in dft.FUNCTIONALS:
                raise TunaError(f"Electronic structure method \"{functional}\" is not supported.")
            xn, cn, dfx, hfx, dfc = dft.FUNCTIONALS[name]
        pts = f64(np.asarray(points).reshape(3, -1))
        wts = f64(np.asarray(weights).reshape(-1))
        self._check(self._L.tf_dft_setup(self._ctx, wts.size, ptr(pts), ptr(wts), dft.X_ID[xn], dft.C_ID[cn], dfx, dfc, float(x_alpha)))
        self.functional = {"name": name, "hfx": hfx, "dfx": dfx, "dfc": dfc, "n_points": int(wts.size)}
        return self.functional

    def dft_vxc(self, P):
        """(V_XC, n_electrons_on_grid, E_X * DFX, E_C * DFC) for a closed-shell density (tuna_scf.py:600-654)."""
        import ctypes
        P = f64(P)
        V = np.zeros_like(P)
        n, ex, ec = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._check(self._L.tf_dft_vxc(self._ctx, ptr(P), ptr(V), ctypes.byref(n), ctypes.byref(ex), ctypes.byref(ec)))
        return V, n.value, ex.value, ec.value

    def dft_vxc_unrestricted(self, P_alpha, P_beta):
        """(V_XC^alpha, V_XC^beta, (n_alpha, n_beta), (E_X,alpha * DFX, E_X,beta * DFX), E_C * DFC) for the spin densities
        (calculate_unrestricted_exchange_correlation_matrix, tuna_scf.py:665-750)."""
        import ctypes
        Pa, Pb = f64(P_alpha), f64(P_beta)
        Va, Vb = np.zeros_like(Pa), np.zeros_like(Pb)
        n, ex = np.zeros(2), np.zeros(2)
        ec = ctypes.c_double()
        self._check(self._L.tf_dft_vxc_unrestricted(self._ctx, ptr(Pa), ptr(Pb), ptr(Va), ptr(Vb), n.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                    ex.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(ec)))
        return Va, Vb, (float(n[0]), float(n[1])), (float(ex[0]), float(ex[1])), ec.value

    def dft_clear(self):
        self._check(self._L.tf_dft_clear(self._ctx))
        self.functional = None

    # ---- post-SCF consumers of the resident tensor ------------------------------------------------
    def ao_to_mo(self, C1, C2=None, C3=None, C4=None) -> np.ndarray:
        """(pq|rs) = sum C1[mu,p] C2[nu,q] C3[la,r] C4[si,s] (mu nu|la si); all four default to C1 (tuna_ci.py:204-255)."""
        Cs = [f64(C1)] + [f64(c) if c is not None else None for c in (C2, C3, C4)]
        Cs = [c if c is not None else Cs[0] for c in Cs]
        n = [c.shape[1] for c in Cs]
        out = np.empty(tuple(n))
        self._check(self._L.tf_ao_to_mo(self._ctx, n[0], ptr(Cs[0]), n[1], ptr(Cs[1]), n[2], ptr(Cs[2]), n[3], ptr(Cs[3]), ptr(out)))
        return out

    def mp2_rhf(self, C, eps, n_occ, n_frozen=0) -> dict:
        """RMP2 correlation energy (tuna_mp.py:834-906): {"E_MP2", "E_OS", "E_SS", "seconds"}."""
        Cm, eps = f64(C), f64(eps)
        import ctypes
        os_, ss, t = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._check(self._L.tf_mp2_rhf(self._ctx, int(n_occ), int(n_frozen), ptr(Cm), ptr(eps), ctypes.byref(os_), ctypes.byref(ss),
                                       ctypes.byref(t)))
        return {"E_MP2": os_.value + ss.value, "E_OS": os_.value, "E_SS": ss.value, "seconds": t.value}

    def mp2_uhf(self, C_alpha, C_beta, eps_alpha, eps_beta, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0) -> dict:
        """UMP2 pair energies from canonical UHF orbitals (tuna_mp.py:987-1117): {"E_aa", "E_bb", "E_ab", "E_SS", "E_OS", "E_MP2",
        "seconds"}, E_SS = E_aa + E_bb, E_OS = E_ab."""
        Ca, Cb, ea, eb = f64(C_alpha), f64(C_beta), f64(eps_alpha), f64(eps_beta)
        if Ca.shape != (self.N, self.N) or Cb.shape != (self.N, self.N) or ea.shape != (self.N,) or eb.shape != (self.N,):
            raise TunaError(f"mp2_uhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        import ctypes
        e = (ctypes.c_double * 3)()
        t = ctypes.c_double()
        self._check(self._L.tf_mp2_uhf(self._ctx, int(n_alpha), int(n_beta), int(n_frozen_alpha), int(n_frozen_beta), ptr(Ca), ptr(Cb), ptr(ea),
                                       ptr(eb), e, ctypes.byref(t)))
        E_aa, E_bb, E_ab = e[0], e[1], e[2]
        return {"E_aa": E_aa, "E_bb": E_bb, "E_ab": E_ab, "E_SS": E_aa + E_bb, "E_OS": E_ab, "E_MP2": E_aa + E_bb + E_ab, "seconds": t.value}

    def mp3_rhf(self, C, eps, n_occ, n_frozen=0) -> dict:
        """Restricted MP3 from canonical RHF orbitals (tuna_mp.py:1410-1470): {"E_OS", "E_SS", "E_MP2", "E_pp", "E_hh", "E_ring", "E_MP3",
        "seconds"}; the MP3 terms are unscaled, E_MP3 = E_pp + E_hh + E_ring; seconds = [wall, MO blocks, ladder, rest]."""
        C, eps = f64(C), f64(eps)
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"mp3_rhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        import ctypes
        e2 = (ctypes.c_double * 2)()
        e3 = (ctypes.c_double * 3)()
        t = (ctypes.c_double * 4)()
        self._check(self._L.tf_mp3_rhf(self._ctx, int(n_occ), int(n_frozen), ptr(C), ptr(eps), e2, e3, t))
        E_OS, E_SS = e2[0], e2[1]
        return {"E_OS": E_OS, "E_SS": E_SS, "E_MP2": E_OS + E_SS, "E_pp": e3[0], "E_hh": e3[1], "E_ring": e3[2],
                "E_MP3": e3[0] + e3[1] + e3[2], "seconds": list(t)}

    def mp4_rhf(self, C, eps, n_occ, n_frozen=0, level="SDQ") -> dict:
        """Restricted MP4(SDQ) or MP4(DQ) from canonical RHF orbitals (tunafock.h: tf_mp4_rhf; tuna_mp.py:1552-1685 without the triples):
        the keys of mp3_rhf, bit for bit its values, plus {"E_S", "E_D", "E_Q", "E_MP4"}, E_MP4 = E_S + E_D + E_Q (E_S is exactly 0.0 for
        level "DQ"); seconds = [wall, MO blocks, ladder (both passes), rest]."""
        C, eps = f64(C), f64(eps)
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"mp4_rhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        if level not in ("SDQ", "DQ"):
            raise TunaError(f"mp4_rhf: level must be \"SDQ\" or \"DQ\", got {level!r}")
        import ctypes
        e2 = (ctypes.c_double * 2)()
        e3 = (ctypes.c_double * 3)()
        e4 = (ctypes.c_double * 3)()
        t = (ctypes.c_double * 4)()
        self._check(self._L.tf_mp4_rhf(self._ctx, 1 if level == "SDQ" else 0, int(n_occ), int(n_frozen), ptr(C), ptr(eps), e2, e3, e4, t))
        E_OS, E_SS = e2[0], e2[1]
        return {"E_OS": E_OS, "E_SS": E_SS, "E_MP2": E_OS + E_SS, "E_pp": e3[0], "E_hh": e3[1], "E_ring": e3[2],
                "E_MP3": e3[0] + e3[1] + e3[2], "E_S": e4[0], "E_D": e4[1], "E_Q": e4[2], "E_MP4": e4[0] + e4[1] + e4[2], "seconds": list(t)}

    def ccd_rhf(self, C, eps, n_occ, n_frozen=0, method="CCD", max_iter=100, conv_delta_E=1e-6, conv_amplitudes=1e-8, use_diis=True,
                max_diis=6, damping=0.0, return_t2=False, allow_unconverged=False) -> dict:
        """Restricted LCCD or CCD from canonical RHF orbitals, iterated on the resident tensor (tunafock.h: tf_ccd_rhf; tuna_cc.py:830-864,
        :915-960, :3004-3161): {"E_corr", "E_MP2", "n_iter", "converged", "table" [n_iter, 3] = step, E_corr, dE, "t2" [o, o, v, v] with
        return_t2, "seconds" = [wall, MO blocks, ladder, rest]}.  Raises TunaError with the code when the iterations do not converge,
        unless allow_unconverged: the dict then holds the last step."""
        C, eps = f64(C), f64(eps)
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"ccd_rhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        if method not in ("LCCD", "CCD"):
            raise TunaError(f"ccd_rhf: method must be \"LCCD\" or \"CCD\", got {method!r}")
        import ctypes
        from ._lib import CcOpts, CcResult
        o, v = int(n_occ) - int(n_frozen), self.N - int(n_occ)
        opts = CcOpts(1 if method == "CCD" else 0, int(max_iter), int(bool(use_diis)), int(max_diis), float(conv_delta_E), float(conv_amplitudes),
                      float(damping))
        table = np.zeros((max(1, int(max_iter)), 3))
        t2 = np.zeros((o, o, v, v)) if return_t2 and o > 0 and v > 0 else None
        res = CcResult()
        res.table, res.t2 = ptr(table), ptr(t2)
        rc = self._L.tf_ccd_rhf(self._ctx, ctypes.byref(opts), int(n_occ), int(n_frozen), ptr(C), ptr(eps), ctypes.byref(res))
        if rc != 0 and not (rc == -4 and allow_unconverged):     # TF_ENOTCONV
            self._check(rc)
        out = {"E_corr": res.e_corr, "E_MP2": res.e_mp2, "n_iter": int(res.n_iter), "converged": bool(res.converged),
               "table": table[:int(res.n_iter)].copy(), "seconds": list(res.seconds)}
        if return_t2:
            out["t2"] = t2
        return out

    CCSD_METHODS = {"LCCSD": 0, "QCISD": 1, "CCSD": 2}    # TF_CCSD_LCCSD, TF_CCSD_QCISD, TF_CCSD_CCSD

    def ccsd_rhf(self, C, eps, n_occ, n_frozen=0, method="CCSD", max_iter=100, conv_delta_E=1e-6, conv_amplitudes=1e-8, use_diis=True,
                 max_diis=6, damping=0.0, return_t1=False, return_t2=False, allow_unconverged=False) -> dict:
        """Restricted LCCSD, QCISD or CCSD from canonical RHF orbitals, iterated on the resident tensor (tunafock.h: tf_ccsd_rhf;
        tuna_cc.py:1020-1063, :1503-1557, :1638-1718, :3004-3161): the dict of ccd_rhf and "E_singles", "E_connected", "E_disconnected"
        (E_corr is their sum; the first is 0.0, the last is 0.0 unless CCSD), "t1_norm" = ||t1||_2, "T1_diagnostic" = t1_norm /
        sqrt(2 (n_occ - n_frozen)) (tuna_cc.py:656-668), "ladder_batches", "t1" [o, v] with return_t1, "t2" [o, o, v, v] with return_t2.
        Raises TunaError with the code when the iterations do not converge, unless allow_unconverged: the dict then holds the last step."""
        C, eps = f64(C), f64(eps)
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"ccsd_rhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        if method not in self.CCSD_METHODS:
            raise TunaError(f"ccsd_rhf: method must be \"LCCSD\", \"QCISD\" or \"CCSD\", got {method!r}")
        import ctypes
        from ._lib import CcOpts, CcsdResult
        o, v = int(n_occ) - int(n_frozen), self.N - int(n_occ)
        opts = CcOpts(self.CCSD_METHODS[method], int(max_iter), int(bool(use_diis)), int(max_diis), float(conv_delta_E), float(conv_amplitudes),
                      float(damping))
        table = np.zeros((max(1, int(max_iter)), 3))
        t1 = np.zeros((o, v)) if return_t1 and o > 0 and v > 0 else None
        t2 = np.zeros((o, o, v, v)) if return_t2 and o > 0 and v > 0 else None
        res = CcsdResult()
        res.table, res.t1, res.t2 = ptr(table), ptr(t1), ptr(t2)
        rc = self._L.tf_ccsd_rhf(self._ctx, ctypes.byref(opts), int(n_occ), int(n_frozen), ptr(C), ptr(eps), ctypes.byref(res))
        if rc != 0 and not (rc == -4 and allow_unconverged):     # TF_ENOTCONV
            self._check(rc)
        out = {"E_corr": res.e_corr, "E_MP2": res.e_mp2, "E_singles": res.e_singles, "E_connected": res.e_connected,
               "E_disconnected": res.e_disconnected, "t1_norm": res.t1_norm,
               "T1_diagnostic": res.t1_norm / np.sqrt(2.0 * o) if o > 0 else 0.0, "n_iter": int(res.n_iter), "converged": bool(res.converged),
               "ladder_batches": int(res.ladder_batches), "table": table[:int(res.n_iter)].copy(), "seconds": list(res.seconds)}
        if return_t1:
            out["t1"] = t1
        if return_t2:
            out["t2"] = t2
        return out

    TRIPLES_KINDS = {"CCSD(T)": 0, "QCISD(T)": 1, "MP4": 2}    # TF_TRIPLES_CCSD_T, TF_TRIPLES_QCISD_T, TF_TRIPLES_MP4

    def triples_rhf(self, C, eps, n_occ, n_frozen=0, kind="CCSD(T)", t1=None, t2=None, return_e_ijk=False) -> dict:
        """The perturbative triples of CCSD(T), QCISD(T) (with the converged t1 [o, v] and t2 [o, o, v, v] of ccsd_rhf) or of full MP4
        (kind "MP4": no amplitudes, t2 = (ia|jb) / D is made inside) from canonical RHF orbitals on the resident tensor (tunafock.h:
        tf_triples_rhf; tuna_cc.py:2688-2758, tuna_mp.py:403-428 and :1605-1637): {"E_T" = "E_connected" + "E_disconnected" (the last
        exactly 0.0 for MP4), "n_triples" = unordered triples sent through the kernels, "e_ijk" [o, o, o] with return_e_ijk (None
        otherwise; symmetric under permutations, E_T is its sum), "seconds" = [wall, MO blocks, triples loop, rest]}."""
        C, eps = f64(C), f64(eps)
        if kind not in self.TRIPLES_KINDS:
            raise TunaError(f"triples_rhf: kind must be \"CCSD(T)\", \"QCISD(T)\" or \"MP4\", got {kind!r}")
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"triples_rhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        o, v = max(0, int(n_occ) - int(n_frozen)), max(0, self.N - int(n_occ))
        if kind == "MP4":
            if t1 is not None or t2 is not None:
                raise TunaError("triples_rhf: kind \"MP4\" makes its own amplitudes: t1 and t2 must be None")
        else:
            if t1 is None or t2 is None:
                raise TunaError(f"triples_rhf: kind {kind!r} needs the amplitudes t1 [{o}, {v}] and t2 [{o}, {o}, {v}, {v}]")
            t1, t2 = f64(t1), f64(t2)
            if t1.shape != (o, v) or t2.shape != (o, o, v, v):
                raise TunaError(f"triples_rhf: amplitudes must be t1 [{o}, {v}] and t2 [{o}, {o}, {v}, {v}], got {t1.shape} and {t2.shape}")
        import ctypes
        from ._lib import TriplesResult
        e_ijk = np.zeros((o, o, o)) if return_e_ijk and o > 0 else None
        res = TriplesResult()
        res.e_ijk = ptr(e_ijk)
        self._check(self._L.tf_triples_rhf(self._ctx, self.TRIPLES_KINDS[kind], int(n_occ), int(n_frozen), ptr(C), ptr(eps), ptr(t1), ptr(t2),
                                           ctypes.byref(res)))
        return {"E_T": res.e_t, "E_connected": res.e_connected, "E_disconnected": res.e_disconnected, "n_triples": int(res.n_triples),
                "e_ijk": e_ijk, "seconds": list(res.seconds)}

    def cis_rhf(self, C, eps, n_occ, n_frozen=0, method="CIS", singlets=True, triplets=True, n_keep=0, dip=None, return_matrices=False) -> dict:
        """Closed-shell CIS or TDHF (RPA) excited states from canonical RHF orbitals on the resident tensor (tunafock.h: tf_cis_rhf;
        tuna_ci.py:1284-1366, :1466-1518): {"dim", "E_singlet", "E_triplet" [dim] ascending (None for a multiplicity that is off),
        "X_singlet", "Y_singlet", "X_triplet", "Y_triplet" [n_keep, o, v] for the lowest n_keep states (Y = 0 for CIS), "tdm" [dim, 3] and
        "osc" [dim] of the singlets with dip = the AO dipole matrices [3, N, N] (None otherwise), "seconds" = [wall, MO blocks, assembly,
        solves]; with return_matrices "M_plus_singlet", "M_plus_triplet" (A + B, or A for CIS) and "M_minus" (A - B, TDHF) [dim, dim]}.
        Raises TunaError with the library's code and message; TF_ELINALG (-5) when TDHF meets an unstable reference."""
        C, eps = f64(C), f64(eps)
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"cis_rhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        if method not in ("CIS", "TDHF", "RPA"):
            raise TunaError(f"cis_rhf: method must be \"CIS\", \"TDHF\" or \"RPA\", got {method!r}")
        if dip is not None:
            dip = f64(dip)
            if dip.shape != (3, self.N, self.N):
                raise TunaError(f"cis_rhf: the dipole matrices must be [3, {self.N}, {self.N}]")
        return self._cis_rhf_call(C, eps, n_occ, n_frozen, method == "CIS", singlets, triplets, n_keep, dip, return_matrices)

    def _cis_rhf_call(self, C, eps, n_occ, n_frozen, tda, singlets, triplets, n_keep, dip, return_matrices, tddft=None):
        """The buffers, the call and the dict of cis_rhf; with tddft = (hfx, P) the call is tf_tddft_rhf."""
        import ctypes
        from ._lib import CisOpts, CisResult, TddftOpts
        o, v = max(0, int(n_occ) - int(n_frozen)), max(0, self.N - int(n_occ))
        dim = o * v
        nk = max(0, min(int(n_keep), dim))
        res = CisResult()
        arrays = {}

        def take(name, shape, wanted=True):
            arrays[name] = np.zeros(shape) if wanted else None
            return ptr(arrays[name])
        res.e_singlet, res.e_triplet = take("E_singlet", dim, singlets), take("E_triplet", dim, triplets)
        for mult, on in (("singlet", singlets), ("triplet", triplets)):
            setattr(res, f"x_{mult}", take(f"X_{mult}", (nk, o, v), on and nk > 0))
            setattr(res, f"y_{mult}", take(f"Y_{mult}", (nk, o, v), on and nk > 0))
        res.tdm, res.osc = take("tdm", (dim, 3), singlets and dip is not None), take("osc", dim, singlets and dip is not None)
        res.m_plus_singlet = take("M_plus_singlet", (dim, dim), return_matrices and singlets)
        res.m_plus_triplet = take("M_plus_triplet", (dim, dim), return_matrices and triplets)
        res.m_minus = take("M_minus", (dim, dim), return_matrices and not tda)
        if tddft is None:
            opts = CisOpts(int(tda), int(bool(singlets)), int(bool(triplets)), int(n_keep))
            self._check(self._L.tf_cis_rhf(self._ctx, ctypes.byref(opts), int(n_occ), int(n_frozen), ptr(C), ptr(eps), ptr(dip), ctypes.byref(res)))
        else:
            hfx, P = tddft
            opts = TddftOpts(int(tda), int(bool(singlets)), int(bool(triplets)), int(n_keep), float(hfx))
            self._check(self._L.tf_tddft_rhf(self._ctx, ctypes.byref(opts), int(n_occ), int(n_frozen), ptr(C), ptr(eps), ptr(P), ptr(dip),
                                             ctypes.byref(res)))
        out = {"dim": int(res.dim), "seconds": list(res.seconds)}
        for name, a in arrays.items():
            if return_matrices or not name.startswith("M_"):
                out[name] = a
        return out

    def tddft_rhf(self, C, eps, P, n_occ, n_frozen=0, method="TDDFT", hfx=None, singlets=True, triplets=True, n_keep=0, dip=None,
                  return_matrices=False) -> dict:
        """Closed-shell TD-DFT ("TDDFT") or its Tamm-Dancoff approximation ("TDA") from canonical Kohn-Sham orbitals, the density P [N, N]
        of the SCF and the functional of dft_setup (tunafock.h: tf_tddft_rhf): the dict of cis_rhf.  hfx = the share of exact exchange,
        by default that of the functional set up.  Local-density functionals only; the null functional with hfx = 1 is TDHF / CIS.
        P = None reaches the library as NULL (TF_EINVAL)."""
        C, eps = f64(C), f64(eps)
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"tddft_rhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        if method not in ("TDDFT", "TDA"):
            raise TunaError(f"tddft_rhf: method must be \"TDDFT\" or \"TDA\", got {method!r}")
        if P is not None:
            P = f64(P)
            if P.shape != (self.N, self.N):
                raise TunaError(f"tddft_rhf: the density must be [{self.N}, {self.N}]")
        if dip is not None:
            dip = f64(dip)
            if dip.shape != (3, self.N, self.N):
                raise TunaError(f"tddft_rhf: the dipole matrices must be [3, {self.N}, {self.N}]")
        if hfx is None:
            hfx = self.functional["hfx"] if getattr(self, "functional", None) else 1.0
        return self._cis_rhf_call(C, eps, n_occ, n_frozen, method == "TDA", singlets, triplets, n_keep, dip, return_matrices, tddft=(hfx, P))

    def xc_kernel_rhf(self, C, P, n_occ, n_frozen=0, return_points=False):
        """(K_XC_singlet, K_XC_triplet) [dim, dim] of the functional of dft_setup for the orbitals C at the closed-shell density P
        (tunafock.h: tf_xc_kernel_rhf; tuna_dft.py:1097-1147); with return_points also f_points [4, n_points] = the floored rho, f_X,
        f_C^singlet, f_C^triplet."""
        C = f64(C)
        if C.shape != (self.N, self.N):
            raise TunaError(f"xc_kernel_rhf: orbitals must be [{self.N}, {self.N}]")
        if P is not None:
            P = f64(P)
            if P.shape != (self.N, self.N):
                raise TunaError(f"xc_kernel_rhf: the density must be [{self.N}, {self.N}]")
        dim = max(0, int(n_occ) - int(n_frozen)) * max(0, self.N - int(n_occ))
        KS, KT = np.zeros((dim, dim)), np.zeros((dim, dim))
        G = self.functional["n_points"] if getattr(self, "functional", None) else 0
        fp = np.zeros((4, G)) if return_points and G else None
        self._check(self._L.tf_xc_kernel_rhf(self._ctx, int(n_occ), int(n_frozen), ptr(C), ptr(P), ptr(KS), ptr(KT), ptr(fp)))
        return (KS, KT, fp) if return_points else (KS, KT)

    def xc_kernel_probe(self, psi_o, psi_v, u_singlet, u_triplet):
        """(K_singlet, K_triplet) [o v, o v] = sum_g u(g) psi_o[i, g] psi_v[a, g] psi_o[j, g] psi_v[b, g] for psi_o [o, G], psi_v [v, G] and
        u_singlet, u_triplet [G] (any values), by the kernel and the slab sum of xc_kernel_rhf (tunafock.h: tf_xc_kernel_probe)."""
        po, pv, us, ut = f64(psi_o), f64(psi_v), f64(u_singlet), f64(u_triplet)
        if po.ndim != 2 or pv.ndim != 2 or po.shape[1] != pv.shape[1] or us.shape != (po.shape[1],) or ut.shape != us.shape:
            raise ValueError(f"xc_kernel_probe: needs psi_o [o, G], psi_v [v, G], u_singlet [G], u_triplet [G], got {po.shape}, {pv.shape}, {us.shape}, {ut.shape}")
        dim = po.shape[0] * pv.shape[0]
        KS, KT = np.full((dim, dim), np.nan), np.full((dim, dim), np.nan)
        self._check(self._L.tf_xc_kernel_probe(self._ctx, po.shape[0], pv.shape[0], po.shape[1], ptr(po), ptr(pv), ptr(us), ptr(ut), ptr(KS), ptr(KT)))
        return KS, KT

    def xc_kernel_timings(self) -> dict:
        """Seconds of the last kernel build by stage (tunafock.h: tf_xc_kernel_timings)."""
        import ctypes
        t = (ctypes.c_double * 4)()
        self._check(self._L.tf_xc_kernel_timings(self._ctx, t))
        return {"psi_gemm": t[0], "point_kernels": t[1], "k_kernel": t[2], "slab_sum": t[3]}

    @staticmethod
    def xc_kernel_plan(dim: int, n_points: int) -> dict:
        """The launch plan of the kernel build, a pure function of (dim, n_points) (tunafock.h: tf_xc_kernel_plan)."""
        import ctypes
        from . import _lib
        out = (ctypes.c_int64 * 8)()
        if _lib.lib().tf_xc_kernel_plan(int(dim), int(n_points), out) != 0:
            raise TunaError("xc_kernel_plan: dim and n_points must be at least 1")
        keys = ("n_b", "n_tiles", "n_slabs", "slab_len", "lds_bytes", "chunk", "slab_min", "tile")
        return dict(zip(keys, (int(x) for x in out)))

    def _uhf_orbitals(self, who, C_alpha, C_beta, eps_alpha, eps_beta):
        Ca, Cb, ea, eb = f64(C_alpha), f64(C_beta), f64(eps_alpha), f64(eps_beta)
        if Ca.shape != (self.N, self.N) or Cb.shape != (self.N, self.N) or ea.shape != (self.N,) or eb.shape != (self.N,):
            raise TunaError(f"{who}: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}] for both spins")
        return Ca, Cb, ea, eb

    def cis_uhf(self, C_alpha, C_beta, eps_alpha, eps_beta, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0, method="CIS", n_keep=0, dip=None,
                return_matrices=False) -> dict:
        """Spin-conserving CIS or TDHF (RPA) excited states of a UHF determinant on the resident tensor (tunafock.h: tf_cis_uhf;
        tuna_ci.py:1377-1455, :1529-1571): {"dim", "dim_alpha" (the compound index holds the alpha block (ia) = i v_alpha + a first, then
        the beta block), "E" [dim] ascending, "X", "Y" [n_keep, dim] of the lowest n_keep states (Y = 0 for CIS; None with n_keep = 0),
        "tdm" [dim, 3] and "osc" [dim] with dip = the AO dipole matrices [3, N, N] (None otherwise), "seconds" = [wall, MO blocks,
        assembly, solves]; with return_matrices "M_plus" (A + B, or A for CIS) and "M_minus" (A - B, TDHF) [dim, dim]}.  Raises TunaError
        with the library's code and message; TF_ELINALG (-5) when TDHF meets an unstable reference."""
        Ca, Cb, ea, eb = self._uhf_orbitals("cis_uhf", C_alpha, C_beta, eps_alpha, eps_beta)
        if method not in ("CIS", "TDHF", "RPA"):
            raise TunaError(f"cis_uhf: method must be \"CIS\", \"TDHF\" or \"RPA\", got {method!r}")
        if dip is not None:
            dip = f64(dip)
            if dip.shape != (3, self.N, self.N):
                raise TunaError(f"cis_uhf: the dipole matrices must be [3, {self.N}, {self.N}]")
        return self._cis_uhf_call(Ca, Cb, ea, eb, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, method == "CIS", n_keep, dip, return_matrices)

    def _cis_uhf_call(self, Ca, Cb, ea, eb, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, tda, n_keep, dip, return_matrices, tddft=None):
        """The buffers, the call and the dict of cis_uhf; with tddft = (hfx, P_alpha, P_beta) the call is tf_tddft_uhf."""
        import ctypes
        from ._lib import UcisOpts, UcisResult, UtddftOpts
        dim = sum(max(0, int(n) - int(nf)) * max(0, self.N - int(n)) for n, nf in ((n_alpha, n_frozen_alpha), (n_beta, n_frozen_beta)))
        nk = max(0, min(int(n_keep), dim))
        res = UcisResult()
        arrays = {}

        def take(name, shape, wanted=True):
            arrays[name] = np.zeros(shape) if wanted else None
            return ptr(arrays[name])
        res.e = take("E", dim)
        res.x, res.y = take("X", (nk, dim), nk > 0), take("Y", (nk, dim), nk > 0)
        res.tdm, res.osc = take("tdm", (dim, 3), dip is not None), take("osc", dim, dip is not None)
        res.m_plus, res.m_minus = take("M_plus", (dim, dim), return_matrices), take("M_minus", (dim, dim), return_matrices and not tda)
        if tddft is None:
            opts = UcisOpts(int(tda), int(n_keep))
            self._check(self._L.tf_cis_uhf(self._ctx, ctypes.byref(opts), int(n_alpha), int(n_beta), int(n_frozen_alpha), int(n_frozen_beta), ptr(Ca),
                                           ptr(Cb), ptr(ea), ptr(eb), ptr(dip), ctypes.byref(res)))
        else:
            hfx, Pa, Pb = tddft
            opts = UtddftOpts(int(tda), int(n_keep), float(hfx))
            self._check(self._L.tf_tddft_uhf(self._ctx, ctypes.byref(opts), int(n_alpha), int(n_beta), int(n_frozen_alpha), int(n_frozen_beta), ptr(Ca),
                                             ptr(Cb), ptr(ea), ptr(eb), ptr(Pa), ptr(Pb), ptr(dip), ctypes.byref(res)))
        out = {"dim": int(res.dim), "dim_alpha": int(res.dim_alpha), "seconds": list(res.seconds)}
        for name, a in arrays.items():
            if return_matrices or not name.startswith("M_"):
                out[name] = a
        return out

    def _spin_densities(self, who, P_alpha, P_beta):
        """The two densities as float64 [N, N]; None stays None and reaches the library as NULL (TF_EINVAL)."""
        out = []
        for P in (P_alpha, P_beta):
            if P is not None:
                P = f64(P)
                if P.shape != (self.N, self.N):
                    raise TunaError(f"{who}: the densities must be [{self.N}, {self.N}]")
            out.append(P)
        return out

    def _default_hfx(self, hfx):
        if hfx is None:
            hfx = self.functional["hfx"] if getattr(self, "functional", None) else 1.0
        return float(hfx)

    def tddft_uhf(self, C_alpha, C_beta, eps_alpha, eps_beta, P_alpha, P_beta, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0, method="TDDFT",
                  hfx=None, n_keep=0, dip=None, return_matrices=False) -> dict:
        """Spin-conserving TD-DFT ("TDDFT") or its Tamm-Dancoff approximation ("TDA") from canonical unrestricted Kohn-Sham orbitals, the
        spin densities of the SCF and the functional of dft_setup (tunafock.h: tf_tddft_uhf): the dict of cis_uhf.  hfx = the share of
        exact exchange, by default that of the functional set up.  Local-density functionals only; the null functional with hfx = 1 is
        cis_uhf bit for bit."""
        Ca, Cb, ea, eb = self._uhf_orbitals("tddft_uhf", C_alpha, C_beta, eps_alpha, eps_beta)
        if method not in ("TDDFT", "TDA"):
            raise TunaError(f"tddft_uhf: method must be \"TDDFT\" or \"TDA\", got {method!r}")
        Pa, Pb = self._spin_densities("tddft_uhf", P_alpha, P_beta)
        if dip is not None:
            dip = f64(dip)
            if dip.shape != (3, self.N, self.N):
                raise TunaError(f"tddft_uhf: the dipole matrices must be [3, {self.N}, {self.N}]")
        return self._cis_uhf_call(Ca, Cb, ea, eb, n_alpha, n_beta, n_frozen_alpha, n_frozen_beta, method == "TDA", n_keep, dip, return_matrices,
                                  tddft=(self._default_hfx(hfx), Pa, Pb))

    def xc_kernel_uhf(self, C_alpha, C_beta, P_alpha, P_beta, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0, return_points=False):
        """K_XC [dim, dim] of the functional of dft_setup in the compound index of cis_uhf (alpha block, then beta block) at the spin
        densities P_alpha, P_beta (tunafock.h: tf_xc_kernel_uhf; tuna_dft.py:1194-1281); with return_points also f_points [7, n_points] =
        rho_alpha, rho_beta (floored), f_X,aa, f_X,bb, f_C,aa, f_C,ab, f_C,bb."""
        Ca, Cb = f64(C_alpha), f64(C_beta)
        if Ca.shape != (self.N, self.N) or Cb.shape != (self.N, self.N):
            raise TunaError(f"xc_kernel_uhf: orbitals must be [{self.N}, {self.N}] for both spins")
        Pa, Pb = self._spin_densities("xc_kernel_uhf", P_alpha, P_beta)
        dim = sum(max(0, int(n) - int(nf)) * max(0, self.N - int(n)) for n, nf in ((n_alpha, n_frozen_alpha), (n_beta, n_frozen_beta)))
        K = np.zeros((dim, dim))
        G = self.functional["n_points"] if getattr(self, "functional", None) else 0
        fp = np.zeros((7, G)) if return_points and G else None
        self._check(self._L.tf_xc_kernel_uhf(self._ctx, int(n_alpha), int(n_beta), int(n_frozen_alpha), int(n_frozen_beta), ptr(Ca), ptr(Cb), ptr(Pa),
                                             ptr(Pb), ptr(K), ptr(fp)))
        return (K, fp) if return_points else K

    def xc_kernel_spin_probe(self, psi_oa, psi_va, psi_ob, psi_vb, u_aa, u_ab, u_bb):
        """K [dim, dim], dim = o_a v_a + o_b v_b, K[p, q] = sum_g u_st(g) psi_o^s[i, g] psi_v^s[a, g] psi_o^t[j, g] psi_v^t[b, g] in the compound
        index of cis_uhf, for psi_oa [o_a, G], psi_va [v_a, G], psi_ob [o_b, G], psi_vb [v_b, G] (a spin may have no rows) and u_aa, u_ab,
        u_bb [G] (any values), by the kernel and the slab sum of xc_kernel_uhf (tunafock.h: tf_xc_kernel_spin_probe)."""
        us = [f64(u) for u in (u_aa, u_ab, u_bb)]
        G = us[0].shape[0] if us[0].ndim == 1 else -1
        ps = [f64(x) if np.size(x) else np.zeros((0, max(G, 0))) for x in (psi_oa, psi_va, psi_ob, psi_vb)]      # no rows: any empty array
        if G < 1 or any(u.shape != (G,) for u in us) or any(x.ndim != 2 or x.shape[1] != G for x in ps):
            raise ValueError("xc_kernel_spin_probe: needs psi_oa [o_a, G], psi_va [v_a, G], psi_ob [o_b, G], psi_vb [v_b, G] and u_aa, u_ab, u_bb [G], "
                             f"got {[x.shape for x in ps]}, {[u.shape for u in us]}")
        oa, va, ob, vb = (x.shape[0] for x in ps)
        dim = oa * va + ob * vb
        K = np.full((dim, dim), np.nan)
        self._check(self._L.tf_xc_kernel_spin_probe(self._ctx, oa, va, ob, vb, G, *(ptr(x) if x.size else None for x in ps), *(ptr(u) for u in us), ptr(K)))
        return K

    def xc_kernel_spin_cols(self, cols: int = 0):
        """The tile shape of this engine's spin-blocked kernel build: 1 = 64 x 64, 2 = 64 x 128, 0 = the library's default (tunafock.h:
        tf_xc_kernel_spin_cols).  Either shape gives the same bits; tools/gpu_utddft_timing.py measures both."""
        self._check(self._L.tf_xc_kernel_spin_cols(self._ctx, int(cols)))
        return self

    @staticmethod
    def xc_kernel_spin_plan(d_alpha: int, d_beta: int, n_points: int) -> dict:
        """The launch plan of the spin-blocked kernel build, a pure function of (d_alpha, d_beta, n_points) (tunafock.h:
        tf_xc_kernel_spin_plan)."""
        import ctypes
        from . import _lib
        out = (ctypes.c_int64 * 8)()
        if _lib.lib().tf_xc_kernel_spin_plan(int(d_alpha), int(d_beta), int(n_points), out) != 0:
            raise TunaError("xc_kernel_spin_plan: d_alpha, d_beta must not be negative, their sum and n_points at least 1")
        keys = ("n_b_alpha", "n_b_beta", "n_tiles", "n_slabs", "slab_len", "lds_bytes", "partial_doubles", "tile_cols")
        return dict(zip(keys, (int(x) for x in out)))

    def _stability(self, call, dim, n_matrices, return_spectra, return_mode):
        import ctypes
        from ._lib import StabilityResult
        res = StabilityResult()
        spectra = np.zeros((n_matrices, dim)) if return_spectra else None
        kappa = np.zeros((2, dim)) if return_mode else None
        res.spectra, res.kappa = ptr(spectra), ptr(kappa)
        self._check(call(ctypes.byref(res)))
        return res, spectra, kappa

    STABILITY_MATRICES_RHF = ("plus_singlet", "plus_triplet", "minus")
    STABILITY_MATRICES_UHF = ("plus", "minus")

    def stability_rhf(self, C, eps, n_occ, n_frozen=0, return_spectra=False, return_mode=False) -> dict:
        """The lowest eigenvalues of the RHF orbital Hessian [[A, B], [B, A]], singlet (restricted rotations) and triplet (unrestricted
        rotations), from eig(A + B) and eig(A - B) (tunafock.h: tf_stability_rhf; tuna_ci.py:926-985): {"dim", "lowest_singlet",
        "lowest_triplet", "source_singlet", "source_triplet" (a name of STABILITY_MATRICES_RHF), "spectra" {name: [dim] ascending} and
        "mode_singlet", "mode_triplet" [o, v] (the normalised orbital rotation of the lowest mode) when asked for, "seconds" = [wall, MO
        blocks, assembly, solves]}.  An unstable reference is a result: nothing is raised."""
        C, eps = f64(C), f64(eps)
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"stability_rhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        o, v = max(0, int(n_occ) - int(n_frozen)), max(0, self.N - int(n_occ))
        return self._stability_restricted(lambda r: self._L.tf_stability_rhf(self._ctx, int(n_occ), int(n_frozen), ptr(C), ptr(eps), r), o, v,
                                          return_spectra, return_mode)

    def _stability_restricted(self, call, o, v, return_spectra, return_mode):
        names = self.STABILITY_MATRICES_RHF
        res, spectra, kappa = self._stability(call, o * v, 3, return_spectra, return_mode)
        return {"dim": int(res.dim), "lowest_singlet": res.lowest[0], "lowest_triplet": res.lowest[1], "source_singlet": names[res.source[0]],
                "source_triplet": names[res.source[1]], "spectra": dict(zip(names, spectra)) if return_spectra else None,
                "mode_singlet": kappa[0].reshape(o, v) if return_mode else None, "mode_triplet": kappa[1].reshape(o, v) if return_mode else None,
                "seconds": list(res.seconds)}

    def stability_uhf(self, C_alpha, C_beta, eps_alpha, eps_beta, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0, return_spectra=False,
                      return_mode=False) -> dict:
        """The lowest eigenvalue of the spin-conserving UHF orbital Hessian from the spin-blocked A + B and A - B (tunafock.h:
        tf_stability_uhf; tuna_ci.py:994-1038): {"dim", "dim_alpha", "lowest", "source" (a name of STABILITY_MATRICES_UHF), "spectra"
        {name: [dim] ascending} and "mode" [dim] (alpha block, then beta block) when asked for, "seconds"}.  Nothing is raised for an
        unstable reference."""
        Ca, Cb, ea, eb = self._uhf_orbitals("stability_uhf", C_alpha, C_beta, eps_alpha, eps_beta)
        dim = sum(max(0, int(n) - int(nf)) * max(0, self.N - int(n)) for n, nf in ((n_alpha, n_frozen_alpha), (n_beta, n_frozen_beta)))
        return self._stability_unrestricted(lambda r: self._L.tf_stability_uhf(self._ctx, int(n_alpha), int(n_beta), int(n_frozen_alpha), int(n_frozen_beta),
                                                                                ptr(Ca), ptr(Cb), ptr(ea), ptr(eb), r), dim, return_spectra, return_mode)

    def _stability_unrestricted(self, call, dim, return_spectra, return_mode):
        names = self.STABILITY_MATRICES_UHF
        res, spectra, kappa = self._stability(call, dim, 2, return_spectra, return_mode)
        return {"dim": int(res.dim), "dim_alpha": int(res.dim_alpha), "lowest": res.lowest[0], "source": names[res.source[0]],
                "spectra": dict(zip(names, spectra)) if return_spectra else None, "mode": kappa[0] if return_mode else None, "seconds": list(res.seconds)}

    def stability_rks(self, C, eps, P, n_occ, n_frozen=0, hfx=None, return_spectra=False, return_mode=False) -> dict:
        """stability_rhf for a restricted Kohn-Sham solution: the exchange blocks scaled by hfx (by default that of the functional set up)
        and 2 K_S / 2 K_T of xc_kernel_rhf at the density P in the singlet / triplet A + B (tunafock.h: tf_stability_rks;
        tuna_ci.py:1049-1106).  The dict of stability_rhf."""
        C, eps = f64(C), f64(eps)
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"stability_rks: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        if P is not None:
            P = f64(P)
            if P.shape != (self.N, self.N):
                raise TunaError(f"stability_rks: the density must be [{self.N}, {self.N}]")
        o, v = max(0, int(n_occ) - int(n_frozen)), max(0, self.N - int(n_occ))
        hfx = self._default_hfx(hfx)
        return self._stability_restricted(lambda r: self._L.tf_stability_rks(self._ctx, hfx, int(n_occ), int(n_frozen), ptr(C), ptr(eps), ptr(P), r), o, v,
                                          return_spectra, return_mode)

    def stability_uks(self, C_alpha, C_beta, eps_alpha, eps_beta, P_alpha, P_beta, n_alpha, n_beta, n_frozen_alpha=0, n_frozen_beta=0, hfx=None,
                      return_spectra=False, return_mode=False) -> dict:
        """stability_uhf for an unrestricted Kohn-Sham solution: the exchange blocks scaled by hfx and 2 K of xc_kernel_uhf at the spin
        densities in A + B (tunafock.h: tf_stability_uks).  The dict of stability_uhf."""
        Ca, Cb, ea, eb = self._uhf_orbitals("stability_uks", C_alpha, C_beta, eps_alpha, eps_beta)
        Pa, Pb = self._spin_densities("stability_uks", P_alpha, P_beta)
        dim = sum(max(0, int(n) - int(nf)) * max(0, self.N - int(n)) for n, nf in ((n_alpha, n_frozen_alpha), (n_beta, n_frozen_beta)))
        hfx = self._default_hfx(hfx)
        return self._stability_unrestricted(lambda r: self._L.tf_stability_uks(self._ctx, hfx, int(n_alpha), int(n_beta), int(n_frozen_alpha),
                                                                                int(n_frozen_beta), ptr(Ca), ptr(Cb), ptr(ea), ptr(eb), ptr(Pa), ptr(Pb), r),
                                            dim, return_spectra, return_mode)

    def cis_d_rhf(self, C, eps, n_occ, n_frozen=0, *, b, omega, triplet) -> dict:
        """CIS(D), the perturbative doubles correction to closed-shell CIS / TDHF states (tunafock.h: tf_cis_d_rhf; tuna_ci.py:1874-1982).
        b [n_states, o, v] (or [o, v] for one state) are the normalised state vectors (CIS: X; TDHF: X + Y), omega their excitation
        energies and triplet their flags (0 = singlet, 1 = triplet).  Returns {"E_D", "E_direct", "E_indirect", "min_denominator"
        [n_states] (E_D = E_direct + E_indirect; min over ijab of |e_i + e_j - e_a - e_b + omega|), "seconds" = [state-independent
        blocks, dressed transformations, kernels and GEMMs]}.  Raises TunaError on a shape mismatch before any device call."""
        C, eps = f64(C), f64(eps)
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"cis_d_rhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        n_occ, n_frozen = int(n_occ), int(n_frozen)
        if not 0 <= n_frozen < n_occ < self.N:
            raise TunaError(f"cis_d_rhf: the windows must satisfy 0 <= n_frozen < n_occ < N, got n_frozen = {n_frozen}, n_occ = {n_occ}, N = {self.N}")
        o, v = n_occ - n_frozen, self.N - n_occ
        b = f64(b)
        if b.ndim == 2:
            b = b[None]
        omega = np.atleast_1d(f64(omega))
        flags = np.atleast_1d(np.asarray(triplet))
        if b.ndim != 3 or b.shape[1:] != (o, v) or b.shape[0] < 1:
            raise TunaError(f"cis_d_rhf: b must be [n_states, {o}, {v}] with n_states >= 1, got {list(b.shape)}")
        n = b.shape[0]
        if omega.shape != (n,) or flags.shape != (n,):
            raise TunaError(f"cis_d_rhf: omega and triplet must have one entry per state ({n}), got {list(omega.shape)} and {list(flags.shape)}")
        if not all(int(f) == f and int(f) in (0, 1) for f in flags.tolist()):
            raise TunaError(f"cis_d_rhf: every triplet flag must be 0 (singlet) or 1 (triplet), got {flags.tolist()}")
        import ctypes
        from ._lib import CisDResult, i32
        b, flags = f64(b), i32(flags)
        res = CisDResult()
        arrays = {k: np.zeros(n) for k in ("E_D", "E_direct", "E_indirect", "min_denominator")}
        res.e_d, res.e_direct, res.e_indirect, res.min_denominator = (ptr(arrays[k]) for k in ("E_D", "E_direct", "E_indirect", "min_denominator"))
        self._check(self._L.tf_cis_d_rhf(self._ctx, n_occ, n_frozen, ptr(C), ptr(eps), n, ptr(b), ptr(omega), ptr(flags), ctypes.byref(res)))
        return dict(arrays, seconds=list(res.seconds))

    def mp2_density_rhf(self, C, eps, n_occ, n_frozen=0, relaxed=False, c_os=1.0, c_ss=1.0) -> dict:
        """The MP2 one-particle density of canonical RHF orbitals, unrelaxed or Z-vector relaxed (tunafock.h: tf_mp2_density_rhf;
        tuna_mp.py:177-279, :908-966).  c_os, c_ss weigh the opposite- and same-spin parts (1, 1: MP2; OSS, SSS: SCS-MP2).  Returns
        {"E_OS", "E_SS", "E_MP2" (unscaled), "P_mo", "P_ao" [N, N] (with the 2 of every occupied orbital), "L", "z" [n_occ, v] (None
        unless relaxed), "seconds" = [wall, MO blocks, ladder, Z-vector, rest]}.  Raises TunaError on a shape or window mismatch before
        any device call."""
        C, eps = f64(C), f64(eps)
        if C.shape != (self.N, self.N) or eps.shape != (self.N,):
            raise TunaError(f"mp2_density_rhf: orbitals must be [{self.N}, {self.N}] and eigenvalues [{self.N}]")
        n_occ, n_frozen = int(n_occ), int(n_frozen)
        if not 0 <= n_frozen < n_occ < self.N:
            raise TunaError(f"mp2_density_rhf: the windows must satisfy 0 <= n_frozen < n_occ < N, got n_frozen = {n_frozen}, n_occ = {n_occ}, N = {self.N}")
        if relaxed and n_frozen != 0:
            raise TunaError(f"mp2_density_rhf: the relaxed density needs n_frozen = 0, got {n_frozen}: the frozen-core Z-vector equations are not built")
        import ctypes
        from ._lib import Mp2DensityOpts, Mp2DensityResult
        opts = Mp2DensityOpts(1 if relaxed else 0, float(c_os), float(c_ss))
        res = Mp2DensityResult()
        P_mo, P_ao = np.zeros((self.N, self.N)), np.zeros((self.N, self.N))
        L = np.zeros((n_occ, self.N - n_occ)) if relaxed else None
        z = np.zeros_like(L) if relaxed else None
        res.P_mo, res.P_ao, res.L, res.z = ptr(P_mo), ptr(P_ao), ptr(L), ptr(z)
        self._check(self._L.tf_mp2_density_rhf(self._ctx, ctypes.byref(opts), n_occ, n_frozen, ptr(C), ptr(eps), ctypes.byref(res)))
        return {"E_OS": res.e_os, "E_SS": res.e_ss, "E_MP2": res.e_os + res.e_ss, "P_mo": P_mo, "P_ao": P_ao, "L": L, "z": z,
                "seconds": list(res.seconds)}

    def natural_orbitals(self, P, X):
        """(occupations, orbitals) of a density matrix P in the AO basis with the Fock orthogonaliser X (tunafock.h: tf_natural_orbitals;
        tuna_mp.py:514-565): eigenpairs of X^-1 P X^-T on the device, occupations descending, orbitals = X vectors (column k)."""
        P, X = f64(P), f64(X)
        n = P.shape[0] if P.ndim == 2 else -1
        if n < 1 or P.shape != (n, n) or X.shape != (n, n):
            raise TunaError(f"natural_orbitals: P and X must be square matrices of one size, got {list(P.shape)} and {list(X.shape)}")
        occ, orb = np.zeros(n), np.zeros((n, n))
        self._check(self._L.tf_natural_orbitals(self._ctx, n, ptr(P), ptr(X), ptr(occ), ptr(orb)))
        return occ, orb

    def mp3_ladder_probe(self, T) -> np.ndarray:
        """Zh[p] = the stored-triangle ladder contraction of the packed tensor with T[p] ([N,N] or [n,N,N], any matrices), by the kernel
        and the batching of mp3_rhf (tunafock.h: tf_mp3_ladder_probe); Z[T] = Zh[T] + Zh[T^T]^T."""
        T = f64(T)
        if T.ndim not in (2, 3) or T.shape[-1] != self.N or T.shape[-2] != self.N:
            raise ValueError(f"mp3_ladder_probe: matrices must be [{self.N},{self.N}] or [n,{self.N},{self.N}], got {T.shape}")
        Zh = np.zeros_like(T)
        self._check(self._L.tf_mp3_ladder_probe(self._ctx, 1 if T.ndim == 2 else T.shape[0], ptr(T), ptr(Zh)))
        return Zh

    def diagonalise(self, F, X):
        """(epsilons, molecular_orbitals) = eigh(sym(X^T F X)), C = X C' on the device (scf:222-250)."""
        F, X = f64(F), f64(X)
        n = F.shape[0]
        eps, Cm = np.zeros(n), np.zeros((n, n))
        self._check(self._L.tf_diagonalise(self._ctx, n, ptr(F), ptr(X), ptr(eps), ptr(Cm)))
        return eps, Cm

    def eigh_stats(self):
        """Counters of the eigensolver paths of this engine's workspace (tunafock.h: tf_eigh_stats)."""
        import ctypes as C
        out = (C.c_int64 * 6)()
        self._check(self._L.tf_eigh_stats(self._ctx, out))
        return dict(zip(("refined_solves", "refinement_steps", "refinement_fallbacks", "blocked_solves", "blocked_declined", "jacobi_fallbacks"),
                        (int(v) for v in out)))

    def jk_path_stats(self):
        """Fock builds of the native cycles over the class-diagonal task list / over the full list (tunafock.h: tf_jk_path_stats)."""
        import ctypes as C
        out = (C.c_int64 * 2)()
        self._check(self._L.tf_jk_path_stats(self._ctx, out))
        return {"class_diagonal_passes": int(out[0]), "full_passes_after_test": int(out[1])}

    def _scf_opts(self, *, conv="medium", max_iter=100, diis=True, max_diis=6, damping="dynamic", damping_factor=0.0, max_damping=0.7,
                  hfx=1.0, n_atom_ao=None):
        N = self.N
        conv_d = SCF_CONVERGENCE[conv] if isinstance(conv, str) else conv
        o = ScfOpts()
        o.max_iter, o.use_diis, o.max_diis = max_iter, int(diis), max_diis
        o.damping = {"none": 0, False: 0, None: 0, "dynamic": 1, True: 1, "static": 2}[damping]
        o.damping_factor, o.max_damping = damping_factor, max_damping
        o.conv_delta_E, o.conv_max_DP = conv_d["delta_E"], conv_d["max_DP"]
        o.conv_rms_DP, o.conv_commutator = conv_d["RMS_DP"], conv_d["commutator"]
        o.hfx = hfx
        n_atom_ao = list(n_atom_ao) if n_atom_ao is not None else [N]
        o.n_atoms = len(n_atom_ao)
        o.n_atom_ao[0] = n_atom_ao[0]
        o.n_atom_ao[1] = n_atom_ao[1] if len(n_atom_ao) > 1 else 0
        return o

    def comm_init(self, uid: bytes, comm_rank: int, comm_size: int):
        """tf_comm_init: attaches an RCCL communicator (collective over the ranks that share the tensor); uid = the 128 bytes rank 0 got
        from Engine.comm_unique_id()."""
        buf = C.create_string_buffer(bytes(uid), 128)
        self._check(self._L.tf_comm_init(self._ctx, buf, int(comm_rank), int(comm_size)))
        return self

    @staticmethod
    def comm_unique_id() -> bytes:
        L = _lib.lib()
        buf = C.create_string_buffer(128)
        rc = L.tf_comm_unique_id(buf)
        if rc != 0:
            raise TunaError(L.tf_last_error(None).decode(), rc)
        return buf.raw

    def comm_attached(self) -> bool:
        return bool(self._L.tf_comm_attached(self._ctx))

    def comm_destroy(self):
        self._check(self._L.tf_comm_destroy(self._ctx))

    def set_allreduce(self, hook):
        """tf_set_allreduce: hook(user, device_ptr, count, stream) -> 0 sums `count` doubles at `device_ptr` over the ranks that share
        the tensor (tuna_amd.distributed.attach_allreduce builds it on torch.distributed); None removes it."""
        from ._lib import ALLREDUCE_FN
        self._allreduce_keepalive = ALLREDUCE_FN(hook) if hook is not None else ALLREDUCE_FN()
        self._check(self._L.tf_set_allreduce(self._ctx, self._allreduce_keepalive, None))
        self.has_allreduce = hook is not None

    def scf_rhf(self, S, T, V, P0, E0, n_occ, V_NN, *, X=None, Fext=None, max_iter=100, **opts):
        N = self.N
        o = self._scf_opts(max_iter=max_iter, **opts)
        r = ScfResult()
        P, Cm, F, eps = np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, N)), np.zeros(N)
        table = np.zeros((max_iter, 7))
        r.P, r.C, r.F, r.eps, r.table = (a.ctypes.data for a in (P, Cm, F, eps, table))
        arrs = [f64(S), f64(T), f64(V), None if Fext is None else f64(Fext), None if X is None else f64(X), f64(P0)]
        rc = self._L.tf_scf_rhf(self._ctx, C.byref(o), *[ptr(a) for a in arrs], float(E0), int(n_occ), float(V_NN),
                                C.byref(r))
        res = {"energy": r.energy, "components": np.array(r.components[:]), "n_iter": r.n_iter, "converged": bool(r.converged),
               "P": P, "C": Cm, "F": F, "epsilons": eps, "table": table[:r.n_iter].copy(), "fock_seconds": r.fock_seconds,
               "eig_seconds": r.eig_seconds, "wall_seconds": r.wall_seconds}
        if rc != 0:
            err = TunaError(self._L.tf_last_error(self._ctx).decode(), rc)
            err.partial = res
            raise err
        return res

    def scf_rhf_batch(self, S, T, V, P0s, E0s, n_occ, V_NN, *, X=None, Fexts=None, max_iter=100, **opts):
        """tf_scf_rhf_batch: several restricted cycles on the resident tensor advanced in lockstep inside the library (the finite-field
        evaluations of energy:315-540); the Fock builds of an iteration go through the tensor together.  Returns the result
        dictionaries of tf_scf_rhf in order, each with "rc"; raises if any cycle failed (err.partial = the list)."""
        N, n = self.N, len(P0s)
        o = self._scf_opts(max_iter=max_iter, **opts)
        res_arr = (ScfResult * n)()
        bufs = []
        for k in range(n):
            P, Cm, F, eps, table = np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, N)), np.zeros(N), np.zeros((max_iter, 7))
            res_arr[k].P, res_arr[k].C, res_arr[k].F, res_arr[k].eps, res_arr[k].table = (a.ctypes.data for a in (P, Cm, F, eps, table))
            bufs.append((P, Cm, F, eps, table))
        P0a = [f64(p) for p in P0s]
        Fa = [None if (Fexts is None or f is None) else f64(f) for f in (Fexts if Fexts is not None else [None] * n)]
        p0_ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in P0a])
        f_ptrs = (C.c_void_p * n)(*[(a.ctypes.data if a is not None else None) for a in Fa])
        E0a = f64(np.asarray(E0s, dtype=np.float64))
        rcs = np.zeros(n, dtype=np.int32)
        passes = np.zeros(2, dtype=np.int64)
        arrs = [f64(S), f64(T), f64(V)]
        Xa = None if X is None else f64(X)
        rc = self._L.tf_scf_rhf_batch(self._ctx, n, C.byref(o), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), f_ptrs, ptr(Xa), p0_ptrs, ptr(E0a),
                                      int(n_occ), float(V_NN), res_arr, ptr(rcs), ptr(passes))
        out = []
        for k in range(n):
            r, (P, Cm, F, eps, table) = res_arr[k], bufs[k]
            out.append({"energy": r.energy, "components": np.array(r.components[:]), "n_iter": r.n_iter, "converged": bool(r.converged),
                        "P": P, "C": Cm, "F": F, "epsilons": eps, "table": table[:r.n_iter].copy(), "fock_seconds": r.fock_seconds,
                        "eig_seconds": r.eig_seconds, "wall_seconds": r.wall_seconds, "rc": int(rcs[k]),
                        "tensor_passes": int(passes[0]), "fock_builds": int(passes[1])})
        if rc != 0:
            err = TunaError(self._L.tf_last_error(self._ctx).decode(), rc)
            err.partial = out
            raise err
        return out

    def scf_uhf(self, S, T, V, P0_alpha, P0_beta, E0, n_alpha, n_beta, V_NN, *, X=None, Fext=None, max_iter=100, **opts):
        """tf_scf_uhf: the unrestricted cycle (scf:1165-1281) on the device; spin quantities come back as pairs (alpha, beta)."""
        N = self.N
        o = self._scf_opts(max_iter=max_iter, **opts)
        r = ScfUhfResult()
        Pt, table = np.zeros((N, N)), np.zeros((max_iter, 7))
        P, Cm, F, eps = np.zeros((2, N, N)), np.zeros((2, N, N)), np.zeros((2, N, N)), np.zeros((2, N))
        r.common.P, r.common.table = Pt.ctypes.data, table.ctypes.data
        for sp in range(2):
            r.P_spin[sp], r.C_spin[sp], r.F_spin[sp], r.eps_spin[sp] = (a[sp].ctypes.data for a in (P, Cm, F, eps))
        arrs = [f64(S), f64(T), f64(V), None if Fext is None else f64(Fext), None if X is None else f64(X), f64(P0_alpha), f64(P0_beta)]
        rc = self._L.tf_scf_uhf(self._ctx, C.byref(o), *[ptr(a) for a in arrs], float(E0), int(n_alpha), int(n_beta), float(V_NN), C.byref(r))
        c = r.common
        res = {"energy": c.energy, "components": np.array(c.components[:]), "n_iter": c.n_iter, "converged": bool(c.converged),
               "P": Pt, "P_spin": P, "C_spin": Cm, "F_spin": F, "epsilons_spin": eps, "table": table[:c.n_iter].copy(),
               "fock_seconds": c.fock_seconds, "eig_seconds": c.eig_seconds, "wall_seconds": c.wall_seconds}
        if rc != 0:
            err = TunaError(self._L.tf_last_error(self._ctx).decode(), rc)
            err.partial = res
            raise err
        return res

    def scf_uks(self, S, T, V, P0_alpha, P0_beta, E0, n_alpha, n_beta, V_NN, *, X=None, Fext=None, max_iter=100, **opts):
        """tf_scf_uks: unrestricted Kohn-Sham with the functional of dft_setup -- the cycle of scf_uhf with V_XC^alpha, V_XC^beta
        (tuna_scf.py:1237-1260); components[3] holds HF + grid exchange, components[4] the correlation energy."""
        N = self.N
        o = self._scf_opts(max_iter=max_iter, **opts)
        r = ScfUhfResult()
        Pt, table = np.zeros((N, N)), np.zeros((max_iter, 7))
        P, Cm, F, eps = np.zeros((2, N, N)), np.zeros((2, N, N)), np.zeros((2, N, N)), np.zeros((2, N))
        r.common.P, r.common.table = Pt.ctypes.data, table.ctypes.data
        for sp in range(2):
            r.P_spin[sp], r.C_spin[sp], r.F_spin[sp], r.eps_spin[sp] = (a[sp].ctypes.data for a in (P, Cm, F, eps))
        arrs = [f64(S), f64(T), f64(V), None if Fext is None else f64(Fext), None if X is None else f64(X), f64(P0_alpha), f64(P0_beta)]
        rc = self._L.tf_scf_uks(self._ctx, C.byref(o), *[ptr(a) for a in arrs], float(E0), int(n_alpha), int(n_beta), float(V_NN), C.byref(r))
        c = r.common
        res = {"energy": c.energy, "components": np.array(c.components[:]), "n_iter": c.n_iter, "converged": bool(c.converged),
               "P": Pt, "P_spin": P, "C_spin": Cm, "F_spin": F, "epsilons_spin": eps, "table": table[:c.n_iter].copy(),
               "fock_seconds": c.fock_seconds, "eig_seconds": c.eig_seconds, "wall_seconds": c.wall_seconds}
        if rc != 0:
            err = TunaError(self._L.tf_last_error(self._ctx).decode(), rc)
            err.partial = res
            raise err
        return res
