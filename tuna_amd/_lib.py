"""ctypes binding of libtunafock.so (include/tunafock.h).  No CPU fallback: if the library or a GPU is
missing, every compute call raises TunaError."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TUNAFOCK_LIB") or os.path.join(HERE, "libtunafock.so")


class TunaError(RuntimeError):
    """Mirror of the reference's TunaError raised by error() (tuna_util.py:933-944)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


class ScfOpts(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("use_diis", C.c_int32), ("max_diis", C.c_int32), ("damping", C.c_int32),
                ("damping_factor", C.c_double), ("max_damping", C.c_double), ("conv_delta_E", C.c_double),
                ("conv_max_DP", C.c_double), ("conv_rms_DP", C.c_double), ("conv_commutator", C.c_double),
                ("hfx", C.c_double), ("n_atom_ao", C.c_int32 * 2), ("n_atoms", C.c_int32)]


class ScfResult(C.Structure):
    _fields_ = [("energy", C.c_double), ("components", C.c_double * 7), ("n_iter", C.c_int32), ("converged", C.c_int32),
                ("P", C.c_void_p), ("C", C.c_void_p), ("eps", C.c_void_p), ("F", C.c_void_p), ("table", C.c_void_p),
                ("fock_seconds", C.c_double), ("eig_seconds", C.c_double), ("wall_seconds", C.c_double)]


class ScfUhfResult(C.Structure):                          # tf_scf_uhf_result
    _fields_ = [("common", ScfResult), ("P_spin", C.c_void_p * 2), ("C_spin", C.c_void_p * 2), ("eps_spin", C.c_void_p * 2),
                ("F_spin", C.c_void_p * 2)]


class CcOpts(C.Structure):                                # tf_cc_opts
    _fields_ = [("method", C.c_int32), ("max_iter", C.c_int32), ("use_diis", C.c_int32), ("max_diis", C.c_int32),
                ("conv_delta_E", C.c_double), ("conv_amplitudes", C.c_double), ("damping", C.c_double)]


class CcResult(C.Structure):                              # tf_cc_result
    _fields_ = [("e_corr", C.c_double), ("e_mp2", C.c_double), ("n_iter", C.c_int32), ("converged", C.c_int32),
                ("table", C.c_void_p), ("t2", C.c_void_p), ("seconds", C.c_double * 4)]


class CcsdResult(C.Structure):                            # tf_ccsd_result
    _fields_ = [("e_corr", C.c_double), ("e_mp2", C.c_double), ("e_singles", C.c_double), ("e_connected", C.c_double),
                ("e_disconnected", C.c_double), ("t1_norm", C.c_double), ("n_iter", C.c_int32), ("converged", C.c_int32),
                ("ladder_batches", C.c_int64), ("table", C.c_void_p), ("t1", C.c_void_p), ("t2", C.c_void_p), ("seconds", C.c_double * 4)]


class TriplesResult(C.Structure):                         # tf_triples_result
    _fields_ = [("e_t", C.c_double), ("e_connected", C.c_double), ("e_disconnected", C.c_double), ("n_triples", C.c_int64),
                ("e_ijk", C.c_void_p), ("seconds", C.c_double * 4)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)     # tf_allreduce_fn

class CisOpts(C.Structure):                               # tf_cis_opts
    _fields_ = [("tda", C.c_int32), ("singlets", C.c_int32), ("triplets", C.c_int32), ("n_keep", C.c_int32)]


class CisResult(C.Structure):                             # tf_cis_result
    _fields_ = [("dim", C.c_int32), ("e_singlet", C.c_void_p), ("e_triplet", C.c_void_p), ("x_singlet", C.c_void_p), ("y_singlet", C.c_void_p),
                ("x_triplet", C.c_void_p), ("y_triplet", C.c_void_p), ("tdm", C.c_void_p), ("osc", C.c_void_p), ("m_plus_singlet", C.c_void_p),
                ("m_plus_triplet", C.c_void_p), ("m_minus", C.c_void_p), ("seconds", C.c_double * 4)]


class TddftOpts(C.Structure):                             # tf_tddft_opts
    _fields_ = [("tda", C.c_int32), ("singlets", C.c_int32), ("triplets", C.c_int32), ("n_keep", C.c_int32), ("hfx", C.c_double)]


class UcisOpts(C.Structure):                              # tf_ucis_opts
    _fields_ = [("tda", C.c_int32), ("n_keep", C.c_int32)]


class UtddftOpts(C.Structure):                            # tf_utddft_opts
    _fields_ = [("tda", C.c_int32), ("n_keep", C.c_int32), ("hfx", C.c_double)]


class UcisResult(C.Structure):                            # tf_ucis_result
    _fields_ = [("dim", C.c_int32), ("dim_alpha", C.c_int32), ("e", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p), ("tdm", C.c_void_p),
                ("osc", C.c_void_p), ("m_plus", C.c_void_p), ("m_minus", C.c_void_p), ("seconds", C.c_double * 4)]


class StabilityResult(C.Structure):                       # tf_stability_result
    _fields_ = [("dim", C.c_int32), ("dim_alpha", C.c_int32), ("n_matrices", C.c_int32), ("source", C.c_int32 * 2), ("lowest", C.c_double * 2),
                ("spectra", C.c_void_p), ("kappa", C.c_void_p), ("seconds", C.c_double * 4)]


class CisDResult(C.Structure):                            # tf_cis_d_result
    _fields_ = [("e_d", C.c_void_p), ("e_direct", C.c_void_p), ("e_indirect", C.c_void_p), ("min_denominator", C.c_void_p),
                ("seconds", C.c_double * 3)]


class Mp2DensityOpts(C.Structure):                        # tf_mp2_density_opts
    _fields_ = [("relaxed", C.c_int32), ("c_os", C.c_double), ("c_ss", C.c_double)]


class Mp2DensityResult(C.Structure):                      # tf_mp2_density_result
    _fields_ = [("e_os", C.c_double), ("e_ss", C.c_double), ("P_mo", C.c_void_p), ("P_ao", C.c_void_p), ("L", C.c_void_p), ("z", C.c_void_p),
                ("seconds", C.c_double * 5)]


EXPORTS = ["tf_create", "tf_destroy", "tf_last_error", "tf_version", "tf_normalize", "tf_set_basis", "tf_get_norms",
           "tf_dims", "tf_get_sph_matrix", "tf_one_electron", "tf_cross_overlap", "tf_build_eri", "tf_eri_storage",
           "tf_copy_eri", "tf_sample_eri", "tf_eri_element", "tf_fock_jk", "tf_fock_jk_device", "tf_scf_rhf", "tf_scf_uhf",
           "tf_orthogonaliser", "tf_eri_timings", "tf_eri_counts", "tf_eri_build_stats", "tf_shard_plan", "tf_jk_profile",
           "tf_jk_profile_read", "tf_diagonalise", "tf_eigh_probe", "tf_eigh_stats", "tf_jk_path_stats", "tf_ao_to_mo", "tf_mp2_rhf", "tf_mp2_uhf", "tf_mp3_rhf", "tf_mp4_rhf", "tf_mp3_ladder_probe", "tf_ccd_rhf", "tf_ccsd_rhf", "tf_triples_rhf", "tf_cis_rhf", "tf_cis_uhf", "tf_stability_rhf", "tf_stability_uhf", "tf_cis_d_rhf", "tf_mp2_density_rhf", "tf_natural_orbitals", "tf_dft_setup", "tf_dft_vxc", "tf_dft_vxc_unrestricted", "tf_scf_uks",
           "tf_dft_clear", "tf_xc_kernel_plan", "tf_xc_kernel_probe", "tf_xc_kernel_rhf", "tf_xc_kernel_timings", "tf_tddft_rhf", "tf_xc_kernel_spin_plan", "tf_xc_kernel_spin_cols", "tf_xc_kernel_spin_probe",
           "tf_xc_kernel_uhf", "tf_tddft_uhf", "tf_stability_rks", "tf_stability_uks", "tf_set_eri_layout", "tf_eri_layout", "tf_shard_plan_pairs", "tf_packed_pad", "tf_eri_flops", "tf_segment_pad", "tf_set_allreduce", "tf_scf_rhf_batch",
           "tf_comm_unique_id", "tf_comm_init", "tf_comm_destroy", "tf_comm_attached"]

_lib = None


def build_library(force: bool = False) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src_dir = os.path.join(HERE, "csrc")
    # force: `make -B` recompiles every object (a library newer than its sources is not trusted: the driver's build check)
    subprocess.check_call(["make", "-j4", "-C", src_dir, "--no-print-directory"] + (["-B"] if force else []))
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TunaError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(tuna_amd has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.tf_create.restype = vp; L.tf_create.argtypes = [ci, ci, ci]
    L.tf_destroy.restype = None; L.tf_destroy.argtypes = [vp]
    L.tf_last_error.restype = C.c_char_p; L.tf_last_error.argtypes = [vp]
    L.tf_version.restype = ci; L.tf_version.argtypes = []
    L.tf_normalize.restype = ci; L.tf_normalize.argtypes = [ci, ci, ci, ci, vp, vp, vp]
    L.tf_set_basis.restype = ci; L.tf_set_basis.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.tf_get_norms.restype = ci; L.tf_get_norms.argtypes = [vp, vp, vp]
    L.tf_dims.restype = ci; L.tf_dims.argtypes = [vp, ip, ip, ip]
    L.tf_get_sph_matrix.restype = ci; L.tf_get_sph_matrix.argtypes = [vp, vp]
    L.tf_one_electron.restype = ci; L.tf_one_electron.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    L.tf_cross_overlap.restype = ci; L.tf_cross_overlap.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    L.tf_build_eri.restype = ci; L.tf_build_eri.argtypes = [vp, ci]
    L.tf_set_eri_layout.restype = ci; L.tf_set_eri_layout.argtypes = [vp, ci]
    L.tf_eri_layout.restype = ci; L.tf_eri_layout.argtypes = [vp]
    L.tf_packed_pad.restype = ci; L.tf_packed_pad.argtypes = []
    L.tf_eri_storage.restype = ci; L.tf_eri_storage.argtypes = [vp, lp, lp, ip, ip]
    L.tf_eri_flops.restype = ci; L.tf_eri_flops.argtypes = [vp, vp]
    L.tf_segment_pad.restype = ci; L.tf_segment_pad.argtypes = []
    L.tf_set_allreduce.restype = ci; L.tf_set_allreduce.argtypes = [vp, ALLREDUCE_FN, vp]
    L.tf_comm_unique_id.restype = ci; L.tf_comm_unique_id.argtypes = [vp]
    L.tf_comm_init.restype = ci; L.tf_comm_init.argtypes = [vp, vp, ci, ci]
    L.tf_comm_destroy.restype = ci; L.tf_comm_destroy.argtypes = [vp]
    L.tf_comm_attached.restype = ci; L.tf_comm_attached.argtypes = [vp]
    L.tf_copy_eri.restype = ci; L.tf_copy_eri.argtypes = [vp, vp]
    L.tf_sample_eri.restype = ci; L.tf_sample_eri.argtypes = [vp, C.c_int64, vp, vp]
    L.tf_eri_element.restype = ci; L.tf_eri_element.argtypes = [vp, vp, vp, vp, vp, vp, dp]
    L.tf_fock_jk.restype = ci; L.tf_fock_jk.argtypes = [vp, ci, vp, vp, vp]
    L.tf_fock_jk_device.restype = ci; L.tf_fock_jk_device.argtypes = [vp, ci, vp, vp, vp, vp]
    L.tf_scf_rhf.restype = ci
    L.tf_scf_rhf.argtypes = [vp, C.POINTER(ScfOpts), vp, vp, vp, vp, vp, vp, cd, ci, cd, C.POINTER(ScfResult)]
    L.tf_scf_rhf_batch.restype = ci; L.tf_scf_rhf_batch.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, cd, vp, vp, vp]
    L.tf_scf_uhf.restype = ci
    L.tf_scf_uhf.argtypes = [vp, C.POINTER(ScfOpts), vp, vp, vp, vp, vp, vp, vp, cd, ci, ci, cd, C.POINTER(ScfUhfResult)]
    L.tf_orthogonaliser.restype = ci; L.tf_orthogonaliser.argtypes = [vp, ci, vp, vp, vp, dp]
    L.tf_eri_timings.restype = ci; L.tf_eri_timings.argtypes = [vp, vp]
    L.tf_eri_counts.restype = ci; L.tf_eri_counts.argtypes = [vp, vp]
    L.tf_eri_build_stats.restype = ci; L.tf_eri_build_stats.argtypes = [vp, C.POINTER(C.c_int64), ci]
    L.tf_shard_plan.restype = ci; L.tf_shard_plan.argtypes = [ci, vp, ci, vp]
    L.tf_shard_plan_pairs.restype = ci; L.tf_shard_plan_pairs.argtypes = [ci, vp, ci, ci, vp]
    L.tf_diagonalise.restype = ci; L.tf_diagonalise.argtypes = [vp, ci, vp, vp, vp, vp]
    L.tf_ao_to_mo.restype = ci; L.tf_ao_to_mo.argtypes = [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp]
    L.tf_mp2_rhf.restype = ci; L.tf_mp2_rhf.argtypes = [vp, ci, ci, vp, vp, dp, dp, dp]
    L.tf_mp2_uhf.restype = ci; L.tf_mp2_uhf.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, dp, dp]
    L.tf_mp3_rhf.restype = ci; L.tf_mp3_rhf.argtypes = [vp, ci, ci, vp, vp, dp, dp, dp]
    L.tf_mp4_rhf.restype = ci; L.tf_mp4_rhf.argtypes = [vp, ci, ci, ci, vp, vp, dp, dp, dp, dp]
    L.tf_mp3_ladder_probe.restype = ci; L.tf_mp3_ladder_probe.argtypes = [vp, ci, vp, vp]
    L.tf_ccd_rhf.restype = ci; L.tf_ccd_rhf.argtypes = [vp, C.POINTER(CcOpts), ci, ci, vp, vp, C.POINTER(CcResult)]
    L.tf_ccsd_rhf.restype = ci; L.tf_ccsd_rhf.argtypes = [vp, C.POINTER(CcOpts), ci, ci, vp, vp, C.POINTER(CcsdResult)]
    L.tf_triples_rhf.restype = ci; L.tf_triples_rhf.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, C.POINTER(TriplesResult)]
    L.tf_cis_rhf.restype = ci; L.tf_cis_rhf.argtypes = [vp, C.POINTER(CisOpts), ci, ci, vp, vp, vp, C.POINTER(CisResult)]
    L.tf_cis_uhf.restype = ci; L.tf_cis_uhf.argtypes = [vp, C.POINTER(UcisOpts), ci, ci, ci, ci, vp, vp, vp, vp, vp, C.POINTER(UcisResult)]
    L.tf_stability_rhf.restype = ci; L.tf_stability_rhf.argtypes = [vp, ci, ci, vp, vp, C.POINTER(StabilityResult)]
    L.tf_stability_uhf.restype = ci; L.tf_stability_uhf.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, C.POINTER(StabilityResult)]
    L.tf_cis_d_rhf.restype = ci; L.tf_cis_d_rhf.argtypes = [vp, ci, ci, vp, vp, ci, vp, vp, vp, C.POINTER(CisDResult)]
    L.tf_mp2_density_rhf.restype = ci; L.tf_mp2_density_rhf.argtypes = [vp, C.POINTER(Mp2DensityOpts), ci, ci, vp, vp, C.POINTER(Mp2DensityResult)]
    L.tf_natural_orbitals.restype = ci; L.tf_natural_orbitals.argtypes = [vp, ci, vp, vp, vp, vp]
    L.tf_dft_setup.restype = ci; L.tf_dft_setup.argtypes = [vp, C.c_int64, vp, vp, ci, ci, cd, cd, cd]
    L.tf_dft_vxc.restype = ci; L.tf_dft_vxc.argtypes = [vp, vp, vp, dp, dp, dp]
    L.tf_dft_vxc_unrestricted.restype = ci; L.tf_dft_vxc_unrestricted.argtypes = [vp, vp, vp, vp, vp, dp, dp, dp]
    L.tf_scf_uks.restype = ci
    L.tf_scf_uks.argtypes = [vp, C.POINTER(ScfOpts), vp, vp, vp, vp, vp, vp, vp, cd, ci, ci, cd, C.POINTER(ScfUhfResult)]
    L.tf_dft_clear.restype = ci; L.tf_dft_clear.argtypes = [vp]
    L.tf_xc_kernel_plan.restype = ci; L.tf_xc_kernel_plan.argtypes = [C.c_int64, C.c_int64, lp]
    L.tf_xc_kernel_probe.restype = ci; L.tf_xc_kernel_probe.argtypes = [vp, ci, ci, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.tf_xc_kernel_rhf.restype = ci; L.tf_xc_kernel_rhf.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
    L.tf_xc_kernel_timings.restype = ci; L.tf_xc_kernel_timings.argtypes = [vp, dp]
    L.tf_xc_kernel_spin_plan.restype = ci; L.tf_xc_kernel_spin_plan.argtypes = [C.c_int64, C.c_int64, C.c_int64, lp]
    L.tf_xc_kernel_spin_cols.restype = ci; L.tf_xc_kernel_spin_cols.argtypes = [vp, ci]
    L.tf_xc_kernel_spin_probe.restype = ci; L.tf_xc_kernel_spin_probe.argtypes = [vp, ci, ci, ci, ci, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tf_xc_kernel_uhf.restype = ci; L.tf_xc_kernel_uhf.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    L.tf_tddft_uhf.restype = ci; L.tf_tddft_uhf.argtypes = [vp, C.POINTER(UtddftOpts), ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, C.POINTER(UcisResult)]
    L.tf_stability_rks.restype = ci; L.tf_stability_rks.argtypes = [vp, C.c_double, ci, ci, vp, vp, vp, C.POINTER(StabilityResult)]
    L.tf_stability_uks.restype = ci; L.tf_stability_uks.argtypes = [vp, C.c_double, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, C.POINTER(StabilityResult)]
    L.tf_tddft_rhf.restype = ci; L.tf_tddft_rhf.argtypes = [vp, C.POINTER(TddftOpts), ci, ci, vp, vp, vp, vp, C.POINTER(CisResult)]
    L.tf_eigh_probe.restype = ci; L.tf_eigh_probe.argtypes = [vp, ci, ci, ci, dp]
    L.tf_eigh_stats.restype = ci; L.tf_eigh_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    L.tf_jk_path_stats.restype = ci; L.tf_jk_path_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    L.tf_jk_profile.restype = ci; L.tf_jk_profile.argtypes = [vp, ci]
    L.tf_jk_profile_read.restype = ci; L.tf_jk_profile_read.argtypes = [vp, dp, lp]
    _lib = L
    return L


def ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)
