/*
 * tunafock.h -- C ABI of libtunafock.so: the MI355X (gfx950) two-electron-integral / Fock-build /
 * SCF engine that stands behind TUNA's integral module and SCF functions.
 *
 * Every entry point is plain C: pointers and sizes only, row-major float64, no torch/NumPy types.
 * Each one names the reference interface it replaces (h-brough/TUNA v0.12.0; "pyx" =
 * TUNA/tuna_integrals/tuna_integral.pyx, "scf" = TUNA/tuna_scf.py, "kernel" = TUNA/tuna_kernel.py).
 * INTEGRATION.md shows the ctypes stubs a TUNA maintainer would add.
 *
 * Conventions
 *   - return value: 0 on success, negative on failure (TF_E*); tf_last_error() has the message.
 *     No exception crosses this boundary.  There is NO CPU fallback: without a usable GPU every
 *     compute entry point fails with TF_ENODEVICE.
 *   - host arrays are caller-owned; device memory is owned by the context; one context per process
 *     (one process per GPU); calls are synchronous unless they take a stream; a context is
 *     thread-compatible, not thread-safe.
 *   - AO order, geometry (atoms on the z axis), normalisation and the Cartesian->spherical
 *     convention are the reference's.
 */
#ifndef TUNAFOCK_H
#define TUNAFOCK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tf_ctx tf_ctx;

enum {
    TF_OK = 0,
    TF_EINVAL = -1,    /* bad argument / call order                              */
    TF_ENODEVICE = -2, /* no HIP device, or HIP runtime error                    */
    TF_ENOMEM = -3,    /* host or device allocation failed (pyx:1120,1290 MemoryError) */
    TF_ENOTCONV = -4,  /* SCF not converged in max_iter (scf:1435)               */
    TF_ELINALG = -5,   /* rocSOLVER/rocBLAS failure                              */
    TF_EGEOM = -6      /* molecule not on the z axis (kernel:386-388)            */
};

/* ---- life cycle -------------------------------------------------------------------------- */

/* One context per process/GPU.  `device` is the HIP device ordinal; (rank, world) select this
 * process's shard of the (ij) shell-pair rows of the ERI tensor; use
 * rank 0 / world 1 for a single GPU.  Returns NULL on failure (see tf_last_error(NULL)). */
tf_ctx *tf_create(int device, int rank, int world);
void tf_destroy(tf_ctx *ctx);
/* Message of the last failure on `ctx` (or of the last failed tf_create when ctx == NULL). */
const char *tf_last_error(const tf_ctx *ctx);
/* ABI version of the library (major*100 + minor). */
int tf_version(void);

/* Stateless, host only: longest-processing-time assignment of weighted blocks to ranks (a generic
 * helper; replaces the `schedule="dynamic"` load balancing of pyx:1314).  owner[n_blocks]. */
int tf_shard_plan(int n_blocks, const int64_t *weight, int world, int32_t *owner);
/* Stateless, host only: the plan tf_build_eri uses.  Bra shell pairs (A >= B, index A(A+1)/2 + B) of
 * n_shells shells with dim[s] output functions each: for every A the B range is cut into `world`
 * contiguous segments of equal weight (stored values of their rows in `layout`), the heaviest
 * segment going to the least loaded rank -- every rank keeps, for each row index i, long runs of
 * consecutive j, which is what the J/K kernel's 8-row groups want.  owner[n_shells (n_shells+1)/2]. */
int tf_shard_plan_pairs(int n_shells, const int32_t *dim, int layout, int world, int32_t *owner);

/* ---- basis: replaces `Basis.__cinit__` / `Basis.normalize` (pyx:144-210) ------------------ */

/* Stateless helper = Basis.normalize for ONE Cartesian AO: fills norm[nprim] and rescales
 * coefs[nprim] in place, exactly as pyx:174-210 does. */
int tf_normalize(int l, int m, int n, int nprim, const double *exps, double *coefs_inout, double *norm_out);

/* The ordered Cartesian AO list, as `form_basis` (tuna_molecule.py:532-587) hands it to the engine:
 * for AO i: origin[3i..3i+2], lmn[3i..3i+2], primitives prim_off[i]..prim_off[i+1]-1 of exps /
 * coefs_raw (un-normalised contraction coefficients).  The engine normalises (a1), groups
 * consecutive AOs into shells, and builds the shell-pair data (pyx:1050-1128). */
int tf_set_basis(tf_ctx *ctx, int n_ao_cart, const double *origin, const int32_t *lmn, const int32_t *prim_off,
                 const double *exps, const double *coefs_raw);
/* Parity hook for a1: per-primitive norm and normalised coefficients, same layout as exps. */
int tf_get_norms(const tf_ctx *ctx, double *norm, double *coefs_normalised);
/* Dimensions after tf_set_basis: Cartesian / spherical AO counts and number of shells. */
int tf_dims(const tf_ctx *ctx, int *n_cart, int *n_sph, int *n_shell);
/* The Cartesian->spherical matrix U [n_sph, n_cart] (kernel:540-649). */
int tf_get_sph_matrix(const tf_ctx *ctx, double *U);

/* ---- one-electron companions: replace calculate_one_electron_integrals (pyx:282-435) and
 *      calculate_cross_basis_overlap_matrix (pyx:626-768) --------------------------------- */

/* S,T,V [n,n]; D,Q [3,n,n] with n = n_sph if spherical else n_cart (transform kernel:495-502).
 * atom_xyz [3*n_atoms] must be on the z axis; D,Q may be NULL. */
int tf_one_electron(tf_ctx *ctx, int n_atoms, const double *atom_xyz, const double *atom_charge,
                    const double *dipole_origin, int spherical, double *S, double *T, double *V, double *D,
                    double *Q);
/* Overlap between the context's basis (rows) and a second AO list (columns), Cartesian, [n1,n2]. */
int tf_cross_overlap(tf_ctx *ctx, int n_ao2, const double *origin2, const int32_t *lmn2, const int32_t *prim_off2,
                     const double *exps2, const double *coefs_raw2, double *S_cross);

/* ---- two-electron integrals: replace calculate_electron_repulsion_integrals (pyx:1267-1355)
 *      + transform_to_spherical_harmonics (kernel:454-529) -------------------------------- */

/* Build this rank's rows of the (ij|kl) tensor on the device.  spherical = 0 is CARTHARM
 * (kernel:481).  The tensor stays resident in HBM in one of three layouts:
 *   TF_LAYOUT_PACKED (default): the 8-fold unique values without the exact zeros of the x/y parity rule, row (i >= j) = the pairs
 *                               (k >= l) <= (i,j) of its parity class -- ~N^4 / 29 x 8 bytes instead of the reference's 8 N^4 (kernel:349);
 *   TF_LAYOUT_TILES:            the same values in the operand order of v_mfma_f64_16x16x4, second index innermost: the fastest Fock
 *                               pass over FOUR OR MORE densities at once (tf_fock_jk with n_dens >= 4, tf_scf_rhf_batch), slower than
 *                               PACKED for one or two;
 *   TF_LAYOUT_ROWS:             rows (i >= j) x full [k][l] -- 4 N^4 bytes (N > 1024, and the round-1 baseline). */
int tf_build_eri(tf_ctx *ctx, int spherical);
#define TF_LAYOUT_AUTO (-1)
#define TF_LAYOUT_ROWS 0
#define TF_LAYOUT_PACKED 1
#define TF_LAYOUT_TILES 2
/* Layout for the next tf_build_eri (TF_LAYOUT_AUTO = packed when the J/K kernel covers N, i.e. N <= 1024). */
int tf_set_eri_layout(tf_ctx *ctx, int layout);
/* Layout of the stored tensor (TF_LAYOUT_ROWS / TF_LAYOUT_PACKED / TF_LAYOUT_TILES), or TF_EINVAL before tf_build_eri. */
int tf_eri_layout(const tf_ctx *ctx);
/* Alignment unit of the packed layout, in doubles: pair (k >= l) sits at tri(k) + l of its tensor row, where
 * tri(k) = sum over m = 1..k of (m rounded up to the unit); tensor rows are rounded up to the unit as well. */
int tf_packed_pad(void);
/* Bytes of HBM holding the stored rows, number of stored rows, row length (leading dimension). */
int tf_eri_storage(const tf_ctx *ctx, int64_t *bytes, int64_t *n_rows, int32_t *n, int32_t *ld);
/* Dense N^4 tensor with all 8 images, as the reference leaves it in `ERI_AO` (caller-allocated,
 * every element written).  Rows owned by other ranks are filled with zeros when world > 1. */
int tf_copy_eri(tf_ctx *ctx, double *host_out);
/* Values at n_idx index quadruples idx[4*q..4*q+3] = (i,j,k,l) (parity/debug at sizes where the
 * dense copy does not fit the host). */
int tf_sample_eri(tf_ctx *ctx, int64_t n_idx, const int32_t *idx, double *values);
/* One contracted Cartesian integral between four AOs given explicitly
 * (calculate_electron_repulsion_integral, pyx:1376-1414).  Arrays describe 4 AOs like tf_set_basis. */
int tf_eri_element(tf_ctx *ctx, const double *origin, const int32_t *lmn, const int32_t *prim_off,
                   const double *exps, const double *coefs_raw, double *value);

/* ---- Fock build: replaces calculate_coulomb_matrix (scf:55-72) and
 *      calculate_exchange_matrix (scf:27-44) --------------------------------------------- */

/* J_ij = sum_kl (ij|kl) P_kl ;  K_ij = sum_kl (il|kj) P_kl  for n_dens densities, host buffers
 * [n_dens,N,N].  With world > 1 the result is this rank's PARTIAL J and K (sum over ranks =
 * full matrices) and the caller all-reduces -- unless a communicator is attached (tf_comm_init
 * below): then the library has summed them over the ranks already. */
int tf_fock_jk(tf_ctx *ctx, int n_dens, const double *P, double *J, double *K);
/* N > 1 ranks: every rank holds the tensor rows of its bra shell pairs, a Fock build gives partial J and K,
 * and ONE all-reduce of the stacked [J;K] completes them.  The native SCF cycles (tf_scf_rhf / tf_scf_uhf) call this hook once per
 * Fock build on a device buffer of `count` doubles; the caller performs sum-all-reduce over its ranks ordered after / before the work
 * on `stream` (tuna_amd: torch.distributed over RCCL, see tuna_amd/distributed.py).  Returns 0 on success.  Without a registered
 * hook the SCF entry points refuse a sharded tensor. */
typedef int (*tf_allreduce_fn)(void *user, double *device_buf, int64_t count, void *stream);
int tf_set_allreduce(tf_ctx *ctx, tf_allreduce_fn fn, void *user);

/* The exchange step inside the library: an RCCL communicator of the ranks that share the tensor (one process per GPU; RCCL over xGMI).
 * Rank 0 calls tf_comm_unique_id and hands the TF_COMM_ID_BYTES bytes to the other ranks by any means (tuna_amd: torch.distributed's
 * store); then EVERY rank calls tf_comm_init (collective).  From then on the native cycles, tf_ao_to_mo / tf_mp2_rhf and
 * tf_fock_jk_device complete their partial sums with ncclAllReduce on the library's (or the caller's) stream -- no host callback per
 * Fock build; a hook registered with tf_set_allreduce is ignored while a communicator is attached.  librccl is loaded at the first call
 * (dlopen): processes that never shard do not pay for it.  The reference has no counterpart. */
#define TF_COMM_ID_BYTES 128
int tf_comm_unique_id(void *id_out);
int tf_comm_init(tf_ctx *ctx, const void *id, int comm_rank, int comm_size);
int tf_comm_destroy(tf_ctx *ctx);
/* 1 when a communicator is attached: tf_fock_jk_device then returns J and K summed over the ranks. */
int tf_comm_attached(const tf_ctx *ctx);

/* Same with device pointers, asynchronous on `stream` (a hipStream_t, may be NULL for the
 * default stream).  Inputs already in HBM; nothing is synchronised or copied.  With the packed
 * layout the densities must be symmetric here (every SCF density is); tf_fock_jk itself also
 * accepts general matrices (it checks on the host and takes a second pass for them). */
int tf_fock_jk_device(tf_ctx *ctx, int n_dens, const double *dP, double *dJ, double *dK, void *stream);

/* ---- SCF: replaces run_self_consistent_field_cycle (scf:1292-1435) for RHF ---------------- */

typedef struct {
    int32_t max_iter;           /* MAXITER, calc:158 (100)                         */
    int32_t use_diis;           /* DIIS / NODIIS, calc:198,100                     */
    int32_t max_diis;           /* DIIS n (6)                                      */
    int32_t damping;            /* 0 = NODAMP, 1 = dynamic (default), 2 = static   */
    double damping_factor;      /* DAMP x (static)                                 */
    double max_damping;         /* MAXDAMP (0.7), calc:159                         */
    double conv_delta_E;        /* thresholds of util:109-116                      */
    double conv_max_DP;
    double conv_rms_DP;
    double conv_commutator;
    double hfx;                 /* HFX_prop, calc:207 (1.0)                        */
    int32_t n_atom_ao[2];       /* AOs on atom A / B (partition_ranges) for the Mulliken damping */
    int32_t n_atoms;
} tf_scf_opts;

typedef struct {
    double energy;              /* E_total = E_elec + V_NN                         */
    double components[7];       /* kinetic, nuc-el, coulomb, exchange, correlation, field, field-gradient (scf:402) */
    int32_t n_iter;
    int32_t converged;
    double *P;                  /* [N,N] caller-allocated, may be NULL             */
    double *C;                  /* [N,N] molecular orbitals                        */
    double *eps;                /* [N]                                             */
    double *F;                  /* [N,N]                                           */
    double *table;              /* [max_iter,7]: step, E_total, dE, rms(DP), max(DP), commutator, damping (scf:105) */
    double fock_seconds;        /* accumulated device time inside the J/K kernels  */
    double eig_seconds;         /* accumulated time in the eigensolver             */
    double wall_seconds;
} tf_scf_result;

/* Runs the RHF cycle of scf:1072-1154 / 1292-1435 with the tensor built by tf_build_eri.
 * S,T,V,Fext (field terms, may be NULL = 0), X = S^-1/2 (kernel:756-816; NULL => computed here),
 * P0 guess density with guess energy E0, n_occ doubly occupied orbitals. */
int tf_scf_rhf(tf_ctx *ctx, const tf_scf_opts *opts, const double *S, const double *T, const double *V,
               const double *Fext, const double *X, const double *P0, double E0, int n_occ, double V_NN,
               tf_scf_result *out);

/* Unrestricted cycle: run_unrestricted_SCF_cycle (scf:1165-1281) inside the same outer loop.  Both spin densities go
 * through the tensor in one fused pass per iteration.  `common` as for tf_scf_rhf (P = total density; C, eps, F unused);
 * the *_spin arrays are the alpha ([0]) and beta ([1]) quantities, caller-allocated, each may be NULL. */
typedef struct {
    tf_scf_result common;
    double *P_spin[2];          /* [N,N]                                           */
    double *C_spin[2];          /* [N,N]                                           */
    double *eps_spin[2];        /* [N]                                             */
    double *F_spin[2];          /* [N,N]                                           */
} tf_scf_uhf_result;
int tf_scf_uhf(tf_ctx *ctx, const tf_scf_opts *opts, const double *S, const double *T, const double *V,
               const double *Fext, const double *X, const double *P0_alpha, const double *P0_beta, double E0,
               int n_alpha, int n_beta, double V_NN, tf_scf_uhf_result *out);
/* Unrestricted Kohn-Sham: the same cycle with V_XC^alpha, V_XC^beta of the iteration's input densities added to the Fock matrices
 * (tuna_scf.py:1237-1260) and the grid's exchange / correlation energies in components[3] / [4].  Arguments as tf_scf_uhf.  Needs a
 * grid set by tf_dft_setup (TF_EINVAL without one) and an unsharded tensor: world > 1 returns TF_EINVAL (no sharded test exists for
 * this path yet).  tf_scf_uhf with a grid set keeps refusing. */
int tf_scf_uks(tf_ctx *ctx, const tf_scf_opts *opts, const double *S, const double *T, const double *V,
               const double *Fext, const double *X, const double *P0_alpha, const double *P0_beta, double E0,
               int n_alpha, int n_beta, double V_NN, tf_scf_uhf_result *out);

/* Several restricted cycles on the SAME tensor advanced in lockstep: what the reference's finite-field drivers run one after the other
 * (tuna_energy.py:315-540: 2, 8 or 12 energy evaluations that differ only in the field term F_fld, kernel:660-677).  Arguments as
 * tf_scf_rhf, with one Fext (may be NULL, or entries NULL), P0, E0 and result per cycle; every cycle follows the iteration order of
 * a run on its own (scf:1072-1154) and stops by its own criteria, but the Fock builds of an iteration go through the tensor together
 * (two densities per pass).  rc_out[c] (may be NULL): return code of cycle c; passes_out (may be NULL): {passes over the tensor,
 * Fock builds}.  Returns 0 or the first non-zero cycle code.  Unsharded tensors, Hartree-Fock only. */
int tf_scf_rhf_batch(tf_ctx *ctx, int n_cycles, const tf_scf_opts *opts, const double *S, const double *T, const double *V,
                     const double *const *Fext, const double *X, const double *const *P0, const double *E0, int n_occ, double V_NN,
                     tf_scf_result *out, int32_t *rc_out, int64_t *passes_out);


/* X = S^-1/2, S^-1 and the smallest overlap eigenvalue (kernel:756-816), host buffers [N,N]. */
int tf_orthogonaliser(tf_ctx *ctx, int n, const double *S, double *X, double *S_inv, double *smallest_eig);

/* ---- Kohn-Sham exchange-correlation (BASELINE config 4) ------------------------- */

/* Hands the molecular integration grid (built by the caller exactly as set_up_integration_grid / build_molecular_grid,
 * tuna_dft.py:94-394, do: xyz [3][n_points], weights [n_points]) to the context, which evaluates every AO and its gradient
 * on it once (construct_basis_functions_on_grid, tuna_dft.py:516-666) and keeps them in HBM.  x_functional: 0 none,
 * 1 Slater, 2 B88, 3 B3 (0.9 B88 + 0.1 Slater); c_functional: 0 none, 1 VWN5, 2 VWN3, 3 LYP, 4 3P (0.81 LYP + 0.19 VWN5),
 * 5 3P with VWN3 ("B3LYP/G"); dfx / dfc = DFX_prop / DFC_prop; x_alpha = X_alpha (2/3).  While a grid is set,
 * tf_scf_rhf runs the restricted Kohn-Sham cycle (opts.hfx = HFX_prop).  Needs tf_build_eri first. */
int tf_dft_setup(tf_ctx *ctx, int64_t n_points, const double *xyz, const double *weights, int x_functional, int c_functional, double dfx,
                 double dfc, double x_alpha);
/* V_XC [N,N] = V_X*DFX + V_C*DFC for the closed-shell density P [N,N] (calculate_restricted_exchange_correlation_matrix,
 * tuna_scf.py:600-654), the grid integral of the density and the scaled exchange / correlation energies. */
int tf_dft_vxc(tf_ctx *ctx, const double *P, double *Vxc, double *n_elec, double *e_x, double *e_c);
/* Spin-resolved V_XC^alpha, V_XC^beta [N,N] for the densities P_alpha, P_beta [N,N] (calculate_unrestricted_exchange_correlation_matrix,
 * tuna_scf.py:665-750), the grid integrals n_elec = {n_alpha, n_beta}, e_x = {E_X,alpha * DFX, E_X,beta * DFX} and e_c = E_C * DFC.
 * Its buffers are allocated on the first call and released with the grid.  Output pointers n_elec, e_x, e_c may be NULL. */
int tf_dft_vxc_unrestricted(tf_ctx *ctx, const double *P_alpha, const double *P_beta, double *Vxc_alpha, double *Vxc_beta,
                            double n_elec[2], double e_x[2], double *e_c);
/* Back to Hartree-Fock. */
int tf_dft_clear(tf_ctx *ctx);

/* ---- consumers of the resident tensor: AO->MO transformation and RMP2 ------------- */

/* out[p,q,r,s] = sum_{mu nu la si} C1[mu,p] C2[nu,q] C3[la,r] C4[si,s] (mu nu|la si)  -- chemists' (pq|rs), host out
 * [n1,n2,n3,n4]; C_k are [N, n_k] row-major host matrices (columns = orbitals).  With all four = the full MO matrix
 * this is transform_ERI_AO_to_MO (tuna_ci.py:204-255); every quarter step is an f64 GEMM (rocBLAS / MFMA).
 * Packed layout: a stored row holds the pairs (la si) <= (mu nu); it is transformed as it lies (one read of every stored value,
 * own rows only) and the other half of the tensor is the transposed result -- two transformations unless (C1, C2) = (C3, C4).
 * world > 1: every rank transforms the rows it owns and the hook of tf_set_allreduce sums the result (all ranks call; without
 * the hook the call is refused, TF_EINVAL). */
int tf_ao_to_mo(tf_ctx *ctx, int n1, const double *C1, int n2, const double *C2, int n3, const double *C3, int n4, const double *C4,
                double *out);
/* Restricted MP2 correlation energy components from canonical orbitals C [N,N], eps [N] (tuna_mp.py:834-906, energy part):
 * *e_os = sum g^2/D, *e_ss = sum g (g - g^T_ab)/D over (ia|jb) with i,j in [n_frozen, n_occ), a,b >= n_occ;
 * E_MP2 = e_os + e_ss.  seconds (may be NULL): wall time of transform + energy.  world > 1: as tf_ao_to_mo (one all-reduce of
 * the (ia|jb) block, then every rank evaluates the same sums). */
int tf_mp2_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *eps, double *e_os, double *e_ss, double *seconds);
/* Unrestricted MP2 pair energies from canonical UHF orbitals C_alpha, C_beta [N,N] and eps_alpha, eps_beta [N] (tuna_mp.py:987-1117,
 * energy part), in spatial orbitals with chemists' (ia|jb) and D = e_i + e_j - e_a - e_b; occupied windows [n_frozen_s, n_s),
 * virtual windows [n_s, N):
 *   e_pairs[0] = E_aa = 1/2 sum_{ij,ab in alpha} (ia|jb) [(ia|jb) - (ib|ja)] / D,  e_pairs[1] = E_bb likewise for beta,
 *   e_pairs[2] = E_ab = sum_{i,a alpha; j,b beta} (ia|jb)^2 / D;   E_SS = E_aa + E_bb, E_OS = E_ab.
 * An empty spin block gives 0 and launches nothing.  TF_EINVAL (the context stays usable) without a tensor, on a NULL pointer, or
 * unless 0 <= n_frozen_s <= n_s < N.  Packed layout with at most 32 occupied orbitals per spin (and 48 together): one pass of the
 * first quarter per spin, the stacked bra [C_occ,a | C_occ,b], the L-transforms of the spin blocks completed in the energy kernel;
 * otherwise the general transformation block by block.  seconds (may be NULL): wall time.  world > 1: as tf_ao_to_mo (the
 * transformed blocks are summed over the ranks before the energy). */
int tf_mp2_uhf(tf_ctx *ctx, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha, const double *C_beta,
               const double *eps_alpha, const double *eps_beta, double e_pairs[3], double *seconds);
/* Restricted MP3 from canonical RHF orbitals C [N,N] and eps [N] (run_restricted_MP3, tuna_mp.py:1410-1470); occupied window
 * [n_frozen, n_occ), virtual window [n_occ, N), D = e_i + e_j - e_a - e_b, t_ijab = (ia|jb) / D, t'_ijab = 2 [2 (ia|jb) - (ib|ja)] / D:
 *   e_mp2 = {E_OS, E_SS}, exactly what tf_mp2_rhf returns for the same orbitals;
 *   e_mp3 = the unscaled terms of E_MP3 = sum t'_ijab X_ijab: [0] particle-particle ladder 1/2 sum_cd t_ijcd (ac|bd), [1] hole-hole
 *           ladder 1/2 sum_kl t_klab (ki|lj), [2] ring terms; E_MP3 is their sum.
 * The ladder never forms (ac|bd): with T_ij = C_v t_ij C_v^T it is 1/2 C_v^T Z_ij C_v, Z_ij = sum (mu lambda|nu sigma) T_ij[lambda][sigma].
 * Packed layout: Z from one pass of a matrix-core kernel over the stored rows per batch of 64 pairs; rows and tiles layouts: Z from
 * the general-density exchange build.  seconds (may be NULL): [0] wall time, [1] MO blocks, [2] ladder, [3] the rest.
 * TF_EINVAL (the context stays usable) without a tensor, on a NULL pointer, unless 0 <= n_frozen < n_occ < N, or with world > 1. */
int tf_mp3_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *eps, double e_mp2[2], double e_mp3[3], double *seconds);
/* Restricted MP4(SDQ) (level 1) or MP4(DQ) (level 0) from canonical RHF orbitals (run_restricted_MP4, tuna_mp.py:1552-1685, without the
 * triples); windows, D, t, t' and X[.] (MP3's operator: 1/2 pp + 1/2 hh + ring) as tf_mp3_rhf, L_pqrs = 2 (pq|rs) - (ps|rq):
 *   e_mp2, e_mp3 = bit for bit what tf_mp3_rhf returns for the same arguments (the same kernels in the same order);
 *   e_mp4 = {E_S, E_D, E_Q}, E_MP4 their sum:
 *     E_D = sum t' X[t2],  t2_ijab = (X[t]_ijab + X[t]_jiba) / D: a second pass of the ladder, hole-hole and ring stages;
 *     E_S = sum t' S,  S_ijab = sum_c t1_jc (ai|bc) - sum_k t1_kb (ai|kj),  t1_ia = -[sum_kld t_klad L_kild - sum_kcd t_kicd L_adkc] / (e_i - e_a)
 *           (exactly 0.0 at level 0).  The integrals with three virtual indices are never formed: the first ladder pass is
 *           back-transformed with C_o as well, [C_o^T Z_ij C_v]_ka = sum_cd (kc|ad) t_ijcd, of which the singles need o^2 v sums;
 *     E_Q = sum t' Q, the six products of t, t and (kc|ld) of tuna_mp.py:1645-1650, as rocBLAS GEMMs.
 * Work space: 13 arrays of o^2 v^2 values (tf_mp3_rhf: 10) and the ladder's batch; nothing with three or four virtual indices.
 * seconds (may be NULL): [0] wall time, [1] MO blocks, [2] ladder (both passes), [3] the rest.
 * TF_EINVAL (the context stays usable) as tf_mp3_rhf, and with a level outside {0, 1}; TF_ENOMEM with the size in the message. */
int tf_mp4_rhf(tf_ctx *ctx, int level, int n_occ, int n_frozen, const double *C, const double *eps, double e_mp2[2], double e_mp3[3], double e_mp4[3],
               double *seconds);
/* The particle-particle ladder contraction of tf_mp3_rhf on its own (instrumentation, tests): T = n matrices [n][N][N] and
 * Zh [n][N][N], host buffers in the caller's AO order,
 *   Zh[p][mu][nu] = sum_{lambda sigma} R_(mu lambda)[nu][sigma] T[p][lambda][sigma],
 * R_(mu lambda) = the stored part of the tensor row (mu lambda) expanded to a symmetric matrix, the row's own pair halved: the
 * contraction with the stored triangle, so that Z[T] = Zh[T] + Zh[T^T]^T with Z[T][mu][nu] = sum (mu lambda|nu sigma) T[lambda][sigma].
 * Runs the batches of 64 matrices through the very routine tf_mp3_rhf calls per batch of pairs; only the permutation between the
 * caller's and the internal AO order is added.  An output element the kernel does not write comes back as a NaN.
 * TF_EINVAL (the context stays usable) without a tensor, with n < 1, on a NULL pointer, on the rows and tiles layouts, or with world > 1. */
int tf_mp3_ladder_probe(tf_ctx *ctx, int n, const double *T, double *Zh);

/* ---- coupled-cluster doubles: replaces calculate_coupled_cluster_energy (tuna_cc.py:2950-3175) for restricted LCCD and CCD ---- */

typedef struct {
    int32_t method;             /* 0 = LCCD (tuna_cc.py:830-864), 1 = CCD (tuna_cc.py:915-960) */
    int32_t max_iter;           /* CORRMAXITER (100)                               */
    int32_t use_diis;           /* DIIS / NODIIS                                   */
    int32_t max_diis;           /* DIIS n (6): amplitude vectors kept              */
    double conv_delta_E;        /* |dE| below this and ...                         */
    double conv_amplitudes;     /* ... ||t - t_old||_2 below this: AMPCONV (1e-8)  */
    double damping;             /* CORRDAMP (0): t <- damping t_old + (1 - damping) t */
} tf_cc_opts;

typedef struct {
    double e_corr;              /* sum [2 (ia|jb) - (ib|ja)] t_ijab of the last step */
    double e_mp2;               /* the same sum for the guess t = (ia|jb) / D: E_OS + E_SS of tf_mp2_rhf */
    int32_t n_iter;
    int32_t converged;
    double *table;              /* [max_iter,3] caller-allocated, may be NULL: step, E_corr, dE */
    double *t2;                 /* [o,o,v,v] caller-allocated, may be NULL: t_ijab of the last step */
    double seconds[4];          /* wall time, MO blocks, ladder (all iterations), the rest */
} tf_cc_result;

/* Restricted LCCD / CCD from canonical RHF orbitals C [N,N] and eps [N]; windows as tf_mp3_rhf: occupied [n_frozen, n_occ), virtual
 * [n_occ, N).  The MO blocks (ia|jb), (ij|ab), (ik|jl) are made once; every iteration is one pass of the AO-direct ladder of tf_mp3_rhf
 * over the current amplitudes (the v^4 block is never formed), rocBLAS GEMMs for the hole-hole and ring terms -- CCD: on the
 * intermediates F_ik, F_ca, W_ijkl, W_icak, W_ciak, which need the same three blocks only -- and one fused update kernel; amplitudes,
 * blocks and the DIIS history stay on the device.  Order of a step (tuna_cc.py:3004-3161): new amplitudes; their energy and dE (the
 * first dE is taken from zero); converged if |dE| < conv_delta_E and ||t - t_old||_2 < conv_amplitudes; otherwise the new amplitudes
 * and t - t_old join the DIIS history (the oldest pair leaves once there are more than max_diis), from step 3 on the amplitudes are
 * extrapolated (B matrix with -1 borders; a singular B clears the history and skips the extrapolation), then damping.
 * TF_ENOTCONV after max_iter steps: table, n_iter, e_corr and t2 then hold the last step.  TF_EINVAL (the context stays usable) without a
 * tensor, on a NULL opts, C, eps or out, unless 0 <= n_frozen < n_occ < N, with max_iter < 1, a method other than 0 and 1, or world > 1.
 * TF_ENOMEM, with the size in the message, when the work space does not fit. */
int tf_ccd_rhf(tf_ctx *ctx, const tf_cc_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps, tf_cc_result *out);

/* ---- coupled-cluster singles and doubles: the same loop for restricted LCCSD, QCISD and CCSD ---- */

#define TF_CCSD_LCCSD 0         /* tuna_cc.py:1020-1063 (the reference's input names CEPA, CEPA0, CEPA(0), CEPA[0] too) */
#define TF_CCSD_QCISD 1         /* tuna_cc.py:1503-1557 */
#define TF_CCSD_CCSD  2         /* tuna_cc.py:1638-1718 */

typedef struct {
    double e_corr;              /* e_singles + e_connected + e_disconnected of the last step */
    double e_mp2;               /* the energy of the guess t2 = (ia|jb) / D: E_OS + E_SS of tf_mp2_rhf */
    double e_singles;           /* sum F_ia t_ia with F = diag(eps): exactly 0.0 */
    double e_connected;         /* sum [2 (ia|jb) - (ib|ja)] t_ijab */
    double e_disconnected;      /* sum [2 (ia|jb) - (ib|ja)] t_ia t_jb (CCSD); exactly 0.0 for LCCSD and QCISD */
    double t1_norm;             /* ||t1||_2 of the last step */
    int32_t n_iter;
    int32_t converged;
    int64_t ladder_batches;     /* batches of 64 pair matrices sent through the ladder stage over the whole call */
    double *table;              /* [max_iter,3] caller-allocated, may be NULL: step, E_corr, dE */
    double *t1;                 /* [o,v] caller-allocated, may be NULL: t_ia of the last step */
    double *t2;                 /* [o,o,v,v] caller-allocated, may be NULL: t_ijab of the last step */
    double seconds[4];          /* wall time, MO blocks, ladder (all iterations), the rest */
} tf_ccsd_result;

/* Restricted LCCSD / QCISD / CCSD from canonical RHF orbitals; opts->method is one of the three codes above, everything else in opts,
 * the windows, the guess t2 = (ia|jb) / D and e_mp2 as tf_ccd_rhf; the guess t1 is zero.  One step is a Jacobi update (new t1 and new t2
 * both from the old pair).  Per step: ONE pass of the AO-direct ladder over the o^2 dressed pair matrices
 *     T_ij = C_v th_ij C_v^T + c_i (C_v t_j)^T + (C_v t_i) c_j^T,   th = t2 (LCCSD, QCISD) or t2 + t1 t1 (CCSD),
 * back-transformed with C_v (the ladder and sum_c (ia|cb) t_jc with its image) and with C_o, C_v (sum_cd (kc|ad) th_ijcd and the t1 parts:
 * the three-virtual terms of the singles, CCSD's t1 parts of W_cdab and its two t1 t1 (oo|vv) / (ov|ov) terms), so
 * ladder_batches == n_iter * ceil(o^2 / 64); tf_ccd_rhf's GEMMs on o^2 v^2, o^3 v and o^4 blocks ((ik|ja) is the one new block, made once);
 * CCSD alone adds per step two AO->MO transformations with t1-dressed coefficients (the t1 parts of W_icak and W_ciak as o^2 v^2 blocks)
 * and one general-density J/K build on C_v t1^T C_o^T (the t1 parts of L_ik and L_ca); one fused singles and one fused doubles update.
 * No array with three or four virtual indices exists, on the device or on the host.  t1 lies behind t2 in every amplitude buffer:
 * the DIIS error vector is the concatenation of t2 - t2_old and t1 - t1_old, both blocks are extrapolated with the same coefficients
 * and damped alike.  Converged if |dE| < conv_delta_E, ||t2 - t2_old||_2 < conv_amplitudes and ||t1 - t1_old||_2 < conv_amplitudes.
 * Work space in arrays of o^2 v^2 values: 11 (LCCSD), 16 (QCISD), 18 (CCSD), three of them o v longer, plus 2 (max(max_diis, 2) + 1) DIIS
 * slots of o^2 v^2 + o v with DIIS, the blocks (ia|jb) and (transiently) (ab|ij) and CCSD's dressed pair of them, three o^3 v and two o^4
 * blocks, and the ladder's batch.  Reductions are per block and summed in block order: two identical calls give identical results.
 * TF_ENOTCONV after max_iter steps: table, n_iter, the energies, t1 and t2 then hold the last step.  TF_EINVAL (the context stays usable),
 * TF_ENOMEM as tf_ccd_rhf; a method outside the three codes is TF_EINVAL. */
int tf_ccsd_rhf(tf_ctx *ctx, const tf_cc_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps, tf_ccsd_result *out);

/* ---- perturbative triples: CCSD(T), QCISD(T) (calculate_restricted_CCSD_T_energy, tuna_cc.py:2688-2758) and the triples of full MP4
 * (run_restricted_MP4, tuna_mp.py:403-428 and :1605-1637) ---- */

#define TF_TRIPLES_CCSD_T  0
#define TF_TRIPLES_QCISD_T 1
#define TF_TRIPLES_MP4     2      /* t1 and t2 must be NULL: t2 = (ia|jb)/D is made inside, V = 0 */

typedef struct {
    double e_t;               /* e_connected + e_disconnected */
    double e_connected;       /* the W·Y part ("[T]") */
    double e_disconnected;    /* the V·Y part; exactly 0.0 for TF_TRIPLES_MP4 */
    int64_t n_triples;        /* unordered triples i >= j >= k sent through the kernels (i = j = k skipped) */
    double *e_ijk;            /* [o,o,o] caller-allocated, may be NULL: every ordered triple filled, e_iii exactly 0.0 */
    double seconds[4];        /* wall, MO blocks incl. (ia|bc), the triples loop, the rest */
} tf_triples_result;

/* The non-iterative triples energy of a closed shell from canonical RHF orbitals and (kinds 0 and 1) converged amplitudes t1 [o,v] and
 * t2 [o,o,v,v] as tf_ccsd_rhf returns them; windows as tf_ccsd_rhf.  In chemists' integrals
 *     X_ijk^abc = sum_f (ia|bf) t2[k,j,c,f] - sum_m (ia|jm) t2[m,k,b,c],   W = the sum of X over the six simultaneous permutations of the
 *     columns (i a), (j b), (k c),   V_ijk^abc = s [(jb|kc) t1[i,a] + (ia|kc) t1[j,b] + (ia|jb) t1[k,c]]  (s = 1, 2; V = 0 for MP4),
 *     e_ijk = 1/3 sum_abc (W + V)^abc (4 W^abc + W^bca + W^cab - 2 W^cba - 2 W^acb - 2 W^bac) / (e_i + e_j + e_k - e_a - e_b - e_c),
 * E_T = the sum of e_ijk over all ordered triples.  e_ijk is the average over the six orderings of the reference's per-triple term: it
 * is symmetric in (i, j, k) (every value is computed once and scattered), the total is the reference's.  t2 need not be symmetric under
 * (ij)(ab); only the equality of kind 2 with the reference's MP4 triples rests on that symmetry, which first-order amplitudes have.
 * Data: (ia|bc) as [i][a][b][c], o v^3 values resident on the device (8.0 GB at N = 400, o = 18), made through the AO->MO transformation
 * in slabs of occupied orbitals and slices of b sized from the free memory; TF_TRIPLES_SLAB=n and TF_TRIPLES_SLICE=n (read per call) allow
 * at most n occupied orbitals per slab and n values of b per slice.  Per unordered triple i >= j >= k (i = j = k skipped: n_triples = o (o + 1) (o + 2) / 6 - o) twelve rocBLAS GEMMs write
 * the six X_pqr of its orderings as [a][b][c], and one fused kernel over unordered triples of 8^3 tiles of (a, b, c) forms W at the six
 * permuted tile positions in LDS (28 KB), applies V and D and leaves one pair of partial sums per workgroup: W never reaches HBM.
 * Partials are summed in block order with a fixed association, triples in loop order with their number of distinct orderings (6 or 3):
 * two identical calls give bit-identical results.  seconds: [0] wall, [1] MO blocks incl. (ia|bc), [2] the triples loop, [3] the rest.
 * Measured on one MI355X, warm, o = 18: N = 200 1.0 s (0.83 ms per triple: the GEMMs 0.72, the fused kernel 0.12 = 2.5 TB/s of reads);
 * N = 400 19 - 21 s = (ia|bc) and the other blocks 7 - 13 s + the loop 7.8 - 7.9 s (7.0 ms per triple, not split further).  Against an independent NumPy loop the
 * largest |d| / S seen is 1.7e-15 at N2/cc-pVTZ (S = the sum of magnitudes of a triple's terms), against the reference program 9e-17 Eh.
 * TF_EINVAL (the context stays usable) without a tensor, on a NULL C, eps or out, unless 0 <= n_frozen < n_occ < N, on a kind outside the
 * three, with world > 1, on a NULL t1 or t2 for kinds 0 and 1 and on a non-NULL t1 or t2 for kind 2.  TF_ENOMEM with the size in the message. */
int tf_triples_rhf(tf_ctx *ctx, int kind, int n_occ, int n_frozen, const double *C, const double *eps, const double *t1 /* [o,v] */,
                   const double *t2 /* [o,o,v,v] */, tf_triples_result *out);

/* ---- excited states: replaces calculate_restricted_single_reference_excited_states and calculate_restricted_transition_dipoles
 * (tuna_ci.py:1284-1366, :1466-1518) for closed-shell CIS and TDHF (RPA) ---- */

typedef struct {
    int32_t tda;                /* 1 = CIS (the matrix A alone), 0 = TDHF / RPA    */
    int32_t singlets;           /* which multiplicities to solve; both 0 is TF_EINVAL */
    int32_t triplets;
    int32_t n_keep;             /* state vectors returned per multiplicity: the lowest n_keep (0 = none; clamped to dim) */
} tf_cis_opts;

typedef struct {
    int32_t dim;                /* o v: states per multiplicity (set by the call; 4 bytes of padding follow) */
    double *e_singlet;          /* [dim] ascending, caller-allocated, may be NULL (left untouched when the multiplicity is off) */
    double *e_triplet;          /* [dim] likewise */
    double *x_singlet;          /* [n_keep][o][v] caller-allocated, may be NULL: X of the lowest states */
    double *y_singlet;          /* [n_keep][o][v] likewise: Y (zeros for CIS) */
    double *x_triplet;
    double *y_triplet;
    double *tdm;                /* [dim][3] may be NULL: transition dipoles of the singlets, x y z; needs dip */
    double *osc;                /* [dim] may be NULL: oscillator strengths of the singlets; needs dip */
    double *m_plus_singlet;     /* [dim][dim] may be NULL: the assembled matrix, A + B (TDHF) or A (CIS), singlet -- tests */
    double *m_plus_triplet;     /* [dim][dim] likewise, triplet */
    double *m_minus;            /* [dim][dim] may be NULL: A - B (TDHF only; untouched for CIS) */
    double seconds[4];          /* wall time, MO blocks, assembly, solves and transition moments */
} tf_cis_result;

/* Closed-shell CIS / TDHF excitation energies, state vectors and transition moments from canonical RHF orbitals C [N,N] and eps [N];
 * windows as tf_mp3_rhf: occupied [n_frozen, n_occ), virtual [n_occ, N); dim = o v, compound index (ia) = i v + a.  With HFX = 1,
 *     singlet: A = Delta + 2 (ia|jb) - (ij|ab), B = 2 (ia|jb) - (ib|ja);   triplet: A = Delta - (ij|ab), B = -(ib|ja),
 * Delta = diag(e_a - e_i), each assembled matrix symmetrised as 1/2 (M + M^T) to the last bit.  The blocks (ia|jb) and (ab|ij) are
 * those of tf_mp3_rhf, on every layout; one kernel pass writes all matrices of the call, then the blocks are freed.
 * CIS: one dsyevd of A per multiplicity; negative eigenvalues are returned as they are.
 * TDHF: A - B = L L^T (dpotrf, once for both multiplicities), the symmetric dim x dim problem [L^T (A + B) L] Z = w^2 Z (dsyevd),
 *     X + Y = L Z / sqrt(w), X - Y = sqrt(w) L^-T Z, so that X.X - Y.Y = 1.  If dpotrf fails or any w^2 <= 0 the RHF reference is
 *     unstable: TF_ELINALG, the message names the multiplicity and the value, no state of that call is valid; the context stays usable.
 * Transition moments of the singlets (dip = the three AO dipole matrices [3][N][N], host): mu_n[c] = sqrt(2) sum_ia (C_o^T D^c C_v)_ia
 *     (X + Y)^n_ia (CIS: the eigenvector), f_n = (2/3) w_n |mu_n|^2.  Triplets have none: the caller's zeros.
 * Nothing is reduced with atomics: two calls give the same bits.
 * Work space: the matrices of the call (CIS 1-2, TDHF 2-3 arrays of dim^2) plus one array of dim^2 ((ij|ab) reordered during the
 * assembly, the triangular products during the TDHF solves), the two blocks until the assembly is done, and rocSOLVER's own.
 * TF_EINVAL (the context stays usable) without a tensor, on a NULL opts, C, eps or out, unless 0 <= n_frozen < n_occ < N, with both
 * multiplicities off, n_keep < 0, tdm or osc without dip, or world > 1.  TF_ENOMEM, with the size in the message. */
int tf_cis_rhf(tf_ctx *ctx, const tf_cis_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps, const double *dip,
               tf_cis_result *out);

/* ---- closed-shell TD-DFT and TDA for the local-density functionals: replaces calculate_restricted_exchange_correlation_kernel_matrices
 * (tuna_dft.py:1097-1147) and the density-functional branch of calculate_A_matrix / calculate_B_matrix (tuna_ci.py:719-845) ---- */

/* The launch plan of the kernel build for dim = o v and n_points grid points, a pure function of the two (no context, no device):
 * out = {64-wide blocks n_b, tiles n_b (n_b + 1) / 2, slabs, slab length, LDS bytes of a workgroup, points per chunk, the shortest slab
 * the plan cuts, tile edge}.  Slab s covers the points [s slab_length, min(n_points, (s + 1) slab_length)).  TF_EINVAL on dim or n_points < 1. */
int tf_xc_kernel_plan(int64_t dim, int64_t n_points, int64_t out[8]);
/* The matrix-core kernel of the build and its slab sum on their own (instrumentation, tests): host psi_o [n_o][n_points],
 * psi_v [n_v][n_points], u_singlet, u_triplet [n_points] (any values), and
 *   K_singlet[(ia)][(jb)] = sum_g u_singlet(g) psi_o[i][g] psi_v[a][g] psi_o[j][g] psi_v[b][g],  (ia) = i n_v + a,   K_triplet likewise,
 * host [dim][dim].  Runs the very routine tf_xc_kernel_rhf and tf_tddft_rhf call; only the transposition of psi to the production
 * operand [n_points][n_o + n_v] is added.  Needs no basis, tensor or grid.  Both results are symmetric to the last bit, and two calls
 * give the same bits: tiles with row block <= column block only, slab partials added in slab order, no atomics.
 * TF_EINVAL (the context stays usable) on a size < 1 or a NULL pointer; TF_ENOMEM with the size in the message. */
int tf_xc_kernel_probe(tf_ctx *ctx, int n_o, int n_v, int64_t n_points, const double *psi_o, const double *psi_v, const double *u_singlet,
                       const double *u_triplet, double *K_singlet, double *K_triplet);
/* K_XC_singlet, K_XC_triplet [dim][dim] (host) of the grid's functional for the orbitals C [N,N], windows as tf_cis_rhf, at the density
 * P [N,N] (the converged closed-shell SCF density, as the reference passes it): rho through the path of tf_dft_vxc, floored at 1e-23,
 *   f_X = 2 d2(n e_X)/dn2,  f_C^S = 2 d2(n e_C)/dn2,  f_C^T = 2 f_mm  (Slater: tuna_xc.py:5956-5983; VWN3: :5994-6061; VWN5: :6151-6236),
 *   u_S = w (DFX f_X + DFC f_C^S),  u_T = w (DFX f_X + DFC f_C^T),  psi = Phi C over the two windows (one GEMM), then the kernel of
 * tf_xc_kernel_probe.  f_points (may be NULL): [4][n_points] = the floored rho, f_X, f_C^S, f_C^T.
 * TF_EINVAL (the context stays usable) without a tensor, without a grid of tf_dft_setup, on a NULL C, P or K, unless
 * 0 <= n_frozen < n_occ < N, with world > 1, or when the grid's functional has a gradient-corrected part (x_functional >= 2 or
 * c_functional >= 3: the message names it).  TF_ENOMEM with the size in the message. */
int tf_xc_kernel_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *P, double *K_singlet, double *K_triplet, double *f_points);
/* Seconds of the last kernel build of the context by stage: {psi GEMM, density and point kernels, K kernel, slab sum}
 * (tf_xc_kernel_probe and tf_xc_kernel_spin_probe: the last two).  The spin-blocked build (tf_xc_kernel_uhf, tf_tddft_uhf,
 * tf_stability_uks) reports its stages in the same slots: both psi GEMMs, both densities and the spin-resolved point kernels, the
 * spin-blocked K kernel, its slab sum. */
int tf_xc_kernel_timings(tf_ctx *ctx, double out[4]);

typedef struct {
    int32_t tda;                /* 1 = TDA (the matrix A alone), 0 = full TD-DFT   */
    int32_t singlets;           /* as tf_cis_opts */
    int32_t triplets;
    int32_t n_keep;
    double hfx;                 /* HFX_prop: the share of exact exchange (1 with the null functional = TDHF, 0 for the pure functionals) */
} tf_tddft_opts;

/* Closed-shell TD-DFT / TDA from canonical Kohn-Sham orbitals: tf_cis_rhf with (calculate_A_matrix / calculate_B_matrix, tuna_ci.py:719-845)
 *     singlet: A = Delta + 2 (ia|jb) - hfx (ij|ab) + K_S,  B = 2 (ia|jb) - hfx (ib|ja) + K_S;
 *     triplet: A = Delta - hfx (ij|ab) + K_T,              B = -hfx (ib|ja) + K_T,
 * K_S, K_T of tf_xc_kernel_rhf at the density P, added after the symmetrisation (they are symmetric to the last bit).  With hfx = 0 the
 * block (ab|ij) is neither built nor read.  With the null functional (tf_dft_setup with x_functional = c_functional = 0) no kernel is
 * built, and with hfx = 1 every output equals tf_cis_rhf's bit for bit.  The solve stages, the transition moments and the rule
 * "unstable reference: TF_ELINALG" are tf_cis_rhf's own code.  seconds as tf_cis_rhf; the kernel build is counted in the assembly slot [2].
 * TF_EINVAL as tf_cis_rhf and tf_xc_kernel_rhf together (no tensor, no grid, a gradient-corrected functional, NULL opts, C, eps, P or
 * out, bad windows, world > 1, hfx not finite).  TF_ENOMEM with the size in the message. */
int tf_tddft_rhf(tf_ctx *ctx, const tf_tddft_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps, const double *P,
                 const double *dip, tf_cis_result *out);

/* ---- unrestricted CIS / TDHF: replaces calculate_unrestricted_single_reference_excited_states (tuna_ci.py:1377-1455) and
 * calculate_unrestricted_transition_dipoles (:1529-1571) ---- */

typedef struct {
    int32_t tda;                /* 1 = CIS (the matrix A alone), 0 = TDHF / RPA */
    int32_t n_keep;             /* state vectors returned: the lowest n_keep (0 = none; clamped to dim) */
} tf_ucis_opts;

typedef struct {
    int32_t dim;                /* d_alpha + d_beta: the number of states (set by the call) */
    int32_t dim_alpha;          /* d_alpha = o_alpha v_alpha: where the beta block of the compound index starts (set by the call) */
    double *e;                  /* [dim] ascending, caller-allocated, may be NULL */
    double *x;                  /* [n_keep][dim] caller-allocated, may be NULL: X of the lowest states, alpha block then beta block */
    double *y;                  /* [n_keep][dim] likewise: Y (zeros for CIS) */
    double *tdm;                /* [dim][3] may be NULL: transition dipoles, x y z; needs dip */
    double *osc;                /* [dim] may be NULL: oscillator strengths; needs dip */
    double *m_plus;             /* [dim][dim] may be NULL: the assembled matrix, A + B (TDHF) or A (CIS) -- tests */
    double *m_minus;            /* [dim][dim] may be NULL: A - B (TDHF only; untouched for CIS) */
    double seconds[4];          /* wall time, MO blocks, assembly, solves and transition moments */
} tf_ucis_result;

/* Spin-conserving CIS / TDHF excitation energies, state vectors and transition moments of a UHF determinant: canonical orbitals
 * C_alpha, C_beta [N,N] and eps_alpha, eps_beta [N].  Per spin s the occupied window is [n_frozen_s, n_s) and the virtual window
 * [n_s, N); d_s = o_s v_s, dim = d_alpha + d_beta.  Compound index: the alpha block first, (ia) = i v_alpha + a, then the beta block,
 * d_alpha + j v_beta + b (the reference's spin-conserving subset of its energy-sorted spin orbitals up to a permutation, which leaves
 * the energies, |mu| and f as they are).  With chemists' integrals and HFX = 1,
 *     A[(ia s),(jb t)] = d_st d_ij d_ab (e_a - e_i) + (ia s|jb t) - d_st (ij|ab),     B[(ia s),(jb t)] = (ia s|jb t) - d_st (ib|ja),
 * each assembled matrix symmetrised as 1/2 (M + M^T) to the last bit; A - B is block-diagonal in spin, its alpha-beta rectangles are
 * exact zeros.  The five MO blocks -- (ia|jb) for aa, bb and ab, (ab|ij) for aa and bb -- come from the general transformation on every
 * tensor layout; one kernel pass writes all matrices of the call, then the blocks are freed.  An empty spin block (o_s = 0 or v_s = 0,
 * the H atom's beta spin) launches nothing.
 * CIS: one dsyevd of A; negative eigenvalues are returned as they are.
 * TDHF: as tf_cis_rhf: A - B = L L^T (dpotrf), [L^T (A + B) L] Z = w^2 Z (dsyevd), X + Y = L Z / sqrt(w), X - Y = sqrt(w) L^-T Z, so that
 *     X.X - Y.Y = 1 over both spins.  If dpotrf fails or any w^2 <= 0 the UHF reference is unstable: TF_ELINALG, the message names the
 *     leading minor or the smallest w^2, no state of that call is valid; the context stays usable.
 * Transition moments (dip = the three AO dipole matrices [3][N][N], host): mu_n[c] = sum_s sum_ia (C_os^T D^c C_vs)_ia (X + Y)^n_ias,
 *     without the sqrt(2) of the restricted singlets; f_n = (2/3) w_n |mu_n|^2.
 * Nothing is reduced with atomics: two calls give the same bits.
 * Work space: the matrices of the call (CIS 1, TDHF 2 arrays of dim^2) plus, during the TDHF solves, one more array of dim^2; until the
 * assembly is done the five blocks (d_a^2 + d_b^2 + d_a d_b values and the two (ij|ab) of o_s^2 v_s^2, each briefly in two orders), and
 * rocSOLVER's own.
 * TF_EINVAL (the context stays usable) without a tensor, on a NULL opts, C_alpha, C_beta, eps_alpha, eps_beta or out, unless
 * 0 <= n_frozen_s <= n_s <= N for both spins, with dim = 0, n_keep < 0, tdm or osc without dip, or world > 1.  TF_ENOMEM, with the
 * size in the message. */
int tf_cis_uhf(tf_ctx *ctx, const tf_ucis_opts *opts, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta,
               const double *C_alpha, const double *C_beta, const double *eps_alpha, const double *eps_beta, const double *dip,
               tf_ucis_result *out);

/* ---- SCF stability analysis: replaces determine_self_consistent_field_stability (tuna_ci.py:852-1106), the STAB keyword ---- */

typedef struct {
    int32_t dim;                /* order of every matrix: o v (RHF), d_alpha + d_beta (UHF) (set by the call) */
    int32_t dim_alpha;          /* UHF: d_alpha; RHF: dim */
    int32_t n_matrices;         /* RHF 3: A + B singlet, A + B triplet, A - B (matrices 0, 1, 2); UHF 2: A + B, A - B (matrices 0, 1) */
    int32_t source[2];          /* the number of the matrix lowest[k] is an eigenvalue of */
    double lowest[2];           /* RHF: the lowest eigenvalue of the singlet and of the triplet Hessian; UHF: lowest[0] = lowest[1] */
    double *spectra;            /* [n_matrices][dim] may be NULL: every matrix's eigenvalues, ascending */
    double *kappa;              /* [2][dim] may be NULL: the normalised eigenvector u of lowest[k] in its matrix, the orbital rotation
                                 * kappa_ia of that mode (the Hessian's vector is (u, u) / sqrt(2) for A + B, (u, -u) / sqrt(2) for A - B) */
    double seconds[4];          /* wall time, MO blocks, assembly, solves */
} tf_stability_result;

/* The lowest eigenvalues of the orbital Hessian [[A, B], [B, A]] of an RHF or UHF determinant, whose spectrum is eig(A + B) u eig(A - B):
 * the matrix of order 2 dim is never formed.  Only the assembly pass of tf_cis_rhf (its matrices A + B singlet, A + B triplet, A - B) or
 * tf_cis_uhf (A + B, A - B) runs, then one dsyevd per matrix -- eigenvalues only unless kappa is asked for.
 *     RHF: lowest[0] = min(l_min(A + B singlet), l_min(A - B))   (restricted, "singlet" rotations)
 *          lowest[1] = min(l_min(A + B triplet), l_min(A - B))   (unrestricted, "triplet" rotations)
 *     UHF: lowest[0] = lowest[1] = min(l_min(A + B), l_min(A - B)) of the spin-blocked matrices (spin-conserving rotations)
 * Windows, index order, layouts and work space as tf_cis_rhf / tf_cis_uhf in their TDHF form, without the extra array of the solves.  An
 * unstable reference is a result, not an error.  Two calls give the same bits.
 * TF_EINVAL (the context stays usable) without a tensor, on a NULL C, eps or out, windows out of range (RHF: 0 <= n_frozen < n_occ < N;
 * UHF: as tf_cis_uhf, dim = 0 included), or world > 1.  TF_ENOMEM, with the size in the message. */
int tf_stability_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *eps, tf_stability_result *out);
int tf_stability_uhf(tf_ctx *ctx, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha,
                     const double *C_beta, const double *eps_alpha, const double *eps_beta, tf_stability_result *out);

/* ---- unrestricted TD-DFT / TDA and the Kohn-Sham stability analysis for the local-density functionals: replaces
 * calculate_unrestricted_exchange_correlation_kernel_matrices (tuna_dft.py:1194-1281), the "UHF" branches of calculate_A_matrix /
 * calculate_B_matrix with K_XC (tuna_ci.py:719-845) and determine_self_consistent_field_stability with K_XC_singlet / K_XC_triplet /
 * K_XC (tuna_ci.py:1049-1106) ---- */

/* The launch plan of the spin-blocked kernel build for d_alpha = o_a v_a, d_beta = o_b v_b and n_points grid points, a pure function of
 * the three (no context, no device): out = {64-wide blocks of the alpha part, of the beta part, tiles, slabs, slab length, LDS bytes of a
 * workgroup, doubles of the slab partials [slabs][dim][dim], columns of a tile (its rows are 64)}.  Blocks are cut per spin:
 * the last alpha block is padded, not continued into beta; a tile is one row block times one column block (the default) or two adjacent
 * column blocks of one spin (tf_xc_kernel_spin_cols), so every tile has one pair of spins and one weight vector, and the tiles listed are
 * those that hold an element with row <= column (64 x 64: n (n + 1) / 2 of n blocks); an empty spin block has no block.  The slab cut is tf_xc_kernel_plan's rule on this tile count.  TF_EINVAL on a negative d, d_alpha + d_beta < 1 or
 * n_points < 1. */
int tf_xc_kernel_spin_plan(int64_t d_alpha, int64_t d_beta, int64_t n_points, int64_t out[8]);
/* The tile shape of the spin-blocked kernel build of this context (instrumentation: tools/gpu_utddft_timing.py measures both): cols = 1
 * for 64 x 64 tiles, 2 for 64 x 128 tiles (two adjacent column blocks of one spin per workgroup), 0 for the library's default, the shape
 * tf_xc_kernel_spin_plan describes.  Either shape gives the same bits.  TF_EINVAL on any other value. */
int tf_xc_kernel_spin_cols(tf_ctx *ctx, int cols);
/* The spin-blocked matrix-core kernel and its slab sum on their own (instrumentation, tests): host psi_oa [o_a][n_points],
 * psi_va [v_a][n_points], psi_ob, psi_vb likewise, u_aa, u_ab, u_bb [n_points] (any values), and K host [dim][dim], dim = o_a v_a + o_b v_b,
 *   K[p][q] = sum_g u_st(g) psi_o^s[i][g] psi_v^s[a][g] psi_o^t[j][g] psi_v^t[b][g],   p = (ia) of spin s, q = (jb) of spin t,
 * in the compound index of tf_cis_uhf (the alpha block first).  The beta-alpha rectangle is the transpose of the alpha-beta one and is
 * never computed.  Runs the very routine tf_xc_kernel_uhf, tf_tddft_uhf and tf_stability_uks call.  Needs no basis, tensor or grid.  An
 * empty spin (o_s v_s = 0) has no tile and its pointers may be NULL.  K is symmetric to the last bit, and two calls give the same bits: no
 * atomics, slab partials added in slab order.  TF_EINVAL (the context stays usable) on a negative size, n_points < 1, dim = 0 or a NULL
 * pointer that is needed; TF_ENOMEM with the size in the message. */
int tf_xc_kernel_spin_probe(tf_ctx *ctx, int o_a, int v_a, int o_b, int v_b, int64_t n_points, const double *psi_oa, const double *psi_va,
                            const double *psi_ob, const double *psi_vb, const double *u_aa, const double *u_ab, const double *u_bb, double *K);
/* K_XC [dim][dim] (host) of the grid's functional for the orbitals C_alpha, C_beta, windows and index order as tf_cis_uhf, at the spin
 * densities P_alpha, P_beta [N,N]: rho_alpha, rho_beta through the path of tf_dft_vxc_unrestricted, floored at 1e-23 each, n their sum,
 *   f_X,ss = 2 f_X(2 rho_s) (the bare Slater function, tuna_xc.py:5956-5983),  f_C,aa / ab / bb the second derivatives of n e_C
 *   (VWN3: tuna_xc.py:6072-6140; VWN5: :6308-6438; zeta clipped to [-1, 1], 1 +- zeta floored at 1e-23 in f''(zeta) only),
 *   u_ss = w (DFX f_X,ss + DFC f_C,ss),  u_ab = w DFC f_C,ab,  psi_s = Phi C_s over the two windows (one GEMM per spin), then the kernel
 * of tf_xc_kernel_spin_probe.  f_points (may be NULL): [7][n_points] = rho_alpha, rho_beta, f_X,aa, f_X,bb, f_C,aa, f_C,ab, f_C,bb.
 * TF_EINVAL (the context stays usable) as tf_cis_uhf's windows (dim = 0 included) and tf_xc_kernel_rhf's grid and functional checks, on
 * a NULL C, P or K, or with world > 1.  TF_ENOMEM with the size in the message.  tf_xc_kernel_timings reports its stages. */
int tf_xc_kernel_uhf(tf_ctx *ctx, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha, const double *C_beta,
                     const double *P_alpha, const double *P_beta, double *K, double *f_points);

typedef struct {
    int32_t tda;                /* 1 = TDA (the matrix A alone), 0 = full TD-DFT */
    int32_t n_keep;             /* as tf_ucis_opts */
    double hfx;                 /* HFX_prop: the share of exact exchange (1 with the null functional = TDHF, 0 for the pure functionals) */
} tf_utddft_opts;

/* Spin-conserving TD-DFT / TDA from canonical unrestricted Kohn-Sham orbitals: tf_cis_uhf with, G = (ia s|jb t), H = (ij|ab), X = (ib|ja),
 *     A = d_st (Delta - hfx H) + G + K,    A + B = d_st (Delta - hfx H - hfx X) + 2 G + 2 K,    A - B = d_st (Delta - hfx H + hfx X),
 * K of tf_xc_kernel_uhf at the densities P_alpha, P_beta, added after the symmetrisation (it is symmetric to the last bit).  With hfx = 0
 * the two (ab|ij) blocks are neither built nor read.  With the null functional no kernel is built, and with hfx = 1 every output equals
 * tf_cis_uhf's bit for bit.  The solve stages, the transition moments and the rule "A +- B not positive definite: TF_ELINALG" are
 * tf_cis_uhf's own code.  seconds as tf_cis_uhf; the kernel build is counted in the assembly slot [2].
 * TF_EINVAL as tf_cis_uhf and tf_xc_kernel_uhf together (hfx not finite included).  TF_ENOMEM with the size in the message. */
int tf_tddft_uhf(tf_ctx *ctx, const tf_utddft_opts *opts, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha,
                 const double *C_beta, const double *eps_alpha, const double *eps_beta, const double *P_alpha, const double *P_beta, const double *dip,
                 tf_ucis_result *out);

/* The stability analysis of a Kohn-Sham solution: tf_stability_rhf / tf_stability_uhf with the exchange blocks scaled by hfx ((ab|ij) not
 * built when hfx = 0) and the kernel in A + B -- restricted: 2 K_S in the singlet and 2 K_T in the triplet matrix (tf_xc_kernel_rhf at the
 * density P); unrestricted: 2 K (tf_xc_kernel_uhf at P_alpha, P_beta).  A - B carries no kernel.  With the null functional and hfx = 1 the
 * results equal the Hartree-Fock routines'.  An unstable solution is a result, not an error.
 * TF_EINVAL as the Hartree-Fock routine and the kernel build together (hfx not finite included).  TF_ENOMEM with the size in the message. */
int tf_stability_rks(tf_ctx *ctx, double hfx, int n_occ, int n_frozen, const double *C, const double *eps, const double *P, tf_stability_result *out);
int tf_stability_uks(tf_ctx *ctx, double hfx, int n_alpha, int n_beta, int n_frozen_alpha, int n_frozen_beta, const double *C_alpha,
                     const double *C_beta, const double *eps_alpha, const double *eps_beta, const double *P_alpha, const double *P_beta,
                     tf_stability_result *out);

/* ---- CIS(D): replaces calculate_restricted_doubles_correction (tuna_ci.py:1874-1982), the perturbative doubles correction of
 * Head-Gordon, Rico, Oumi and Lee to closed-shell CIS / TDHF states ---- */

typedef struct {
    double *e_d, *e_direct, *e_indirect;   /* [n_states], caller-allocated; e_d = e_direct + e_indirect */
    double *min_denominator;               /* [n_states] may be NULL: min over ijab of |D_ijab + omega| */
    double seconds[3];                     /* state-independent blocks; dressed transformations; kernels and GEMMs */
} tf_cis_d_result;

/* The (D) correction of n_states states of tf_cis_rhf's spectrum from canonical RHF orbitals C [N,N] and eps [N]; windows as tf_mp3_rhf:
 * occupied [n_frozen, n_occ), virtual [n_occ, N).  Per state: b [o][v], normalised (CIS: the eigenvector; TDHF: X + Y), its excitation
 * energy omega, and triplet = 0 (singlet) or 1.  With D_ijab = e_i + e_j - e_a - e_b, t = (ia|jb) / D and s = 1 / (D + omega):
 *     M[iajb] = (i~ a|jb) - sum_k b_ka (ki|jb),   C~_o = C_v b^T,   u_S[ijab] = M[iajb] + M[jbia],   u_T[ijab] = M[iajb] - M[jbia]
 *     e_direct = sum s u_S[ijab] (u_S[ijab] - 1/2 u_S[jiab])                              (singlet)
 *              = 1/2 sum s (u_S[ijab]^2 - u_S[ijab] u_S[jiab] + u_T[ijab]^2)              (triplet)
 *     e_indirect = sum_ia b_ia y_ia - sum_ija b_ia b_ja Goo_ij - sum_iab b_ia b_ib Gvv_ba,   L = 2 (jb|kc) - (jc|kb),
 *     Goo_ij = sum_kbc L_jkbc t_ikbc,   Gvv_ba = sum_jkc L_jkbc t_jkac,   y = (2 t_ikac - t_ikca) (L b)  (singlet),   t_ikca ((jc|kb) b)  (triplet)
 * No block with three virtual indices is formed: per state one AO->MO transformation with the dressed occupied orbitals ((i~ a|jb), as
 * tf_ao_to_mo makes it, on every tensor layout), one GEMM on (ki|jb), one fused pass over M (16 x 16 tiles of (a, b) per pair (i, j),
 * the two transposed elements gathered through LDS) and two to four matrix-vector products.  States are processed one after the other
 * by the same calls, the per-block partial sums are added in block order and nothing is reduced with atomics: a state's three numbers
 * are the same bits alone, in any batch and in two calls.
 * Work space: 5 arrays of o^2 v^2 values ((ia|jb), t, 2 t - t', L, M) plus 2 inside a transformation on the packed and tiles layouts,
 * and (ki|jb) of o^3 v.
 * Measured on one MI355X: 114 states of seven systems within 4.2e-16 Eh of the reference program's E_D on every layout; N = 400, o = 18,
 * warm: 0.04 - 0.14 s for the state-independent blocks (two machines), then 0.022 s (transformation) + 0.002 s (kernels and GEMMs) per state.
 * TF_EINVAL (the context stays usable) without a tensor, on a NULL C, eps, b, omega, triplet, out, e_d, e_direct or e_indirect, with
 * n_states < 1, a flag outside {0, 1}, unless 0 <= n_frozen < n_occ < N, or world > 1.  TF_ENOMEM, with the size in the message. */
int tf_cis_d_rhf(tf_ctx *ctx, int n_occ, int n_frozen, const double *C, const double *eps, int n_states,
                 const double *b /* [n_states][o][v] */, const double *omega /* [n_states] */,
                 const int32_t *triplet /* [n_states], 0 or 1 */, tf_cis_d_result *out);

/* ---- MP2 densities: replaces the density part of run_restricted_MP2 (tuna_mp.py:908-966), calculate_restricted_relaxed_MP2_density_matrix
 * (:177-279) and calculate_natural_orbitals (:514-565) ---- */

typedef struct {
    int32_t relaxed;                       /* 0: unrelaxed; 1: Z-vector relaxed (needs n_frozen = 0) */
    double c_os, c_ss;                     /* weights of the opposite- and same-spin parts: 1, 1 for MP2; OSS, SSS for SCS-MP2 */
} tf_mp2_density_opts;

typedef struct {
    double e_os, e_ss;                     /* the unscaled MP2 components, as tf_mp2_rhf returns them */
    double *P_mo;                          /* [N][N] may be NULL: the density in the MO basis, with the 2 of every occupied orbital */
    double *P_ao;                          /* [N][N] may be NULL: C P_mo C^T */
    double *L, *z;                         /* [n_occ][v] may be NULL, written by a relaxed call: the Lagrangian and the Z-vector */
    double seconds[5];                     /* wall; MO blocks; ladder; Z-vector (assembly, dpotrf, dpotrs); rest */
} tf_mp2_density_result;

/* The MP2 one-particle density of canonical RHF orbitals C [N,N], eps [N]; windows as tf_mp3_rhf: occupied [n_frozen, n_occ), virtual
 * [n_occ, N).  With D = e_i + e_j - e_a - e_b, tOS = -2 (ia|jb) / D, tSS = [(ia|jb) - (ib|ja)] / D:
 *     P_ij = -1/2 c_os sum_kab tOS_kiab tOS_kjab - c_ss sum_kab tSS_kiab tSS_kjab      (occupied window)
 *     P_ab = +1/2 c_os sum_ijc tOS_ijbc tOS_ijac + c_ss sum_ijc tSS_ijbc tSS_ijac      (virtual window)
 * plus 2 on the diagonal of every occupied orbital.  A relaxed call (n_frozen = 0) adds z_ia / 2 to both occupied-virtual blocks, where
 * (A + B) z = -L with the singlet A + B of tf_cis_rhf, w = c_os 2 (ia|jb) / D + c_ss 2 [(ia|jb) - (ib|ja)] / D and
 *     L_ia = 2 sum_jbc w_ijbc (ab|jc) - 2 sum_jkb w_jkab (ji|kb) + [C_o^T (4 J[P_src] - 2 K[P_src]) C_v]_ia,   P_src = C P^(2) C^T.
 * No block with three virtual indices is formed: the first term is one pass of the AO-direct ladder of tf_mp3_rhf on w, back-transformed
 * with the occupied coefficients as tf_mp4_rhf's singles are; the second is a GEMM over (ji|kb); the third one J/K build.  The system is
 * solved by rocSOLVER dpotrf / dpotrs.  A + B that is not positive definite -- a singlet-unstable RHF solution -- is TF_ELINALG, the
 * message names the leading minor, nothing of that call is valid and the context stays usable.  Every reduction has one owner and a
 * fixed order, rocBLAS runs without atomics: two calls return the same bits.  All three tensor layouts.
 * Work space: relaxed at most 6 arrays of o^2 v^2 values at a time -- (ia|jb), (ab|ij), tOS, tSS and w in two layouts; after the
 * unrelaxed stage the ladder's Y, then the transposed (ij|ab) and the (o v)^2 of A + B stand where the amplitudes stood -- plus the
 * ladder's batch; unrelaxed 3 arrays.
 * Measured on one MI355X against the reference program's densities of six systems (MP2 and SCS-MP2, both kinds, every layout): P within
 * 3.3e-15 (MO basis) and 6.5e-14 (AO basis), z within 6.6e-15; N = 400, o = 18, warm: relaxed 1.31 s (MO blocks 0.67 s, ladder 0.57 s,
 * Z-vector 0.03 s), unrelaxed 0.037 s.
 * TF_EINVAL (the context stays usable) without a tensor, on a NULL opts, C, eps or out, unless 0 <= n_frozen < n_occ < N, on a relaxed
 * call with n_frozen > 0 or without any output array, or world > 1.  TF_ENOMEM, with the size in the message. */
int tf_mp2_density_rhf(tf_ctx *ctx, const tf_mp2_density_opts *opts, int n_occ, int n_frozen, const double *C, const double *eps,
                       tf_mp2_density_result *out);

/* Natural orbitals of a density P [n,n] (AO basis) with the Fock orthogonaliser X [n,n]: eigenpairs of X^-1 P X^-T by the context's
 * eigensolver on the device (X^-1 by dgetrf / dgetri), occ [n] in descending order, orbitals [n,n] = X vectors, column k with occ[k].
 * Needs no tensor.  TF_EINVAL on a NULL pointer or n < 1, TF_ELINALG on a singular X or an eigensolver failure. */
int tf_natural_orbitals(tf_ctx *ctx, int n, const double *P, const double *X, double *occ, double *orbitals);

/* eps[N], C[N,N] = eigenpairs of the Fock matrix in the orthogonalised basis, C = X C' (diagonalise_Fock_matrix,
 * scf:222-250): rocBLAS dgemm + rocSOLVER dsyevd; host buffers. */
int tf_diagonalise(tf_ctx *ctx, int n, const double *F, const double *X, double *eps, double *C);

/* ---- instrumentation ------------------------------------------------------------------- */

/* Device-side seconds of the last tf_build_eri broken down by stage:
 * [0] total, [1] primitive/contracted Cartesian kernel, [2] ket transform, [3] bra transform+store. */
int tf_eri_timings(const tf_ctx *ctx, double *seconds4);
/* Work counters of the last tf_build_eri: [0] shell quartets, [1] primitive shell quartets,
 * [2] Cartesian component quartets. */
int tf_eri_counts(const tf_ctx *ctx, int64_t *counts3);
/* The reference algorithm's floating-point operation count for the quartets the last tf_build_eri evaluated (SURVEY.md section 8d(ii):
 * per primitive AO quartet that passes the parity test pyx:1324-1327, 8 x the inner terms of the loop nest pyx:1179-1217 plus the
 * Boys / R table cost 6 (L+1) + 3 (L+1)^2 / 2 + 60).  The device kernels factorise the sums and execute fewer operations; the
 * figure prices the build against the FP64 vector peak. */
int tf_eri_flops(const tf_ctx *ctx, double *nominal_flops);
/* Launch structure of the last tf_build_eri (instrumentation, tests): host counters incremented where the launches are made, no
 * device work and no synchronisation.  out[i] for i < n gets counter i of the list below (0 beyond TF_ERI_STAT_COUNT); TF_EINVAL on a
 * NULL pointer or n < 0.  A slab is one run of this rank's bra shell pairs through generation, ket and bra transform (TF_SLAB_MB,
 * TF_SLAB_ROWS); the family counters count kernel launches and add up to TF_ERI_STAT_LAUNCHES (TF_ERI_STAT_TEAM_FLAT counts launches
 * already counted under their team size). */
enum {
    TF_ERI_STAT_SLABS = 0,
    TF_ERI_STAT_LAUNCHES,             /* launches of ERI generation kernels, every family below                                   */
    TF_ERI_STAT_TEAM16,               /* eri_team_kernel, 16 / 64 / 256 lanes per shell quartet (per-class mode, packed or tiles)  */
    TF_ERI_STAT_TEAM64,
    TF_ERI_STAT_TEAM256,
    TF_ERI_STAT_TEAM_FLAT,            /* ... of those, launches that walk the flat component lists                                 */
    TF_ERI_STAT_TEAMC,                /* eri_teamc_kernel over task lists (small-problem mode, TF_ERI_TEAMC=1)                     */
    TF_ERI_STAT_CFACT_UNCONTRACTED,   /* eri_cfact_kernel (small-problem mode): both groups uncontracted                           */
    TF_ERI_STAT_CFACT_CONTRACTED,     /* ... a contracted group, no families                                                       */
    TF_ERI_STAT_CFACT_GTAB,           /* ... G, X and Z tables in global memory ((hh|hh)-sized quartets)                           */
    TF_ERI_STAT_CFACT_KET_FAMILIES,   /* ... families of ket pairs (general contractions)                                          */
    TF_ERI_STAT_CFACT_BOTH_FAMILIES,  /* ... families on both sides                                                                */
    TF_ERI_STAT_CFACT_BRA_FAMILIES,   /* ... families of bra pairs (TF_ERI_BRA_FAMILIES=1)                                         */
    TF_ERI_STAT_COMPONENT_LANE,       /* the component-per-lane kernel of the small-problem mode (TF_ERI_GENERIC_OLD, oversized LDS) */
    TF_ERI_STAT_MULTI,                /* eri_multi_kernel (per-class mode: several small uncontracted quartets per workgroup)      */
    TF_ERI_STAT_FACT,                 /* eri_fact_kernel (per-class mode: uncontracted, factor tables in LDS)                      */
    TF_ERI_STAT_CLASS_STAGED,         /* eri_class_kernel with the Hermite tables staged in LDS (per-class mode)                   */
    TF_ERI_STAT_CLASS_UNSTAGED,       /* eri_class_kernel reading them from global memory                                          */
    TF_ERI_STAT_COUNT
};
int tf_eri_build_stats(const tf_ctx *ctx, int64_t *out, int n);
/* Alignment unit (in doubles) of the stored segments of the packed, parity-blocked tensor layout. */
int tf_segment_pad(void);

/* Seconds per symmetric eigensolve (random n x n matrix) of the solver variants considered for a12
 * (0 = rocsolver dsyevd, 1 = dsyev, 2 = dsyevj); instrumentation only. */
int tf_eigh_probe(tf_ctx *ctx, int n, int variant, int reps, double *seconds);

/* Counters of the context's eigensolver paths since tf_create (instrumentation, tests): out[0] solves by eigenvector refinement,
 * out[1] refinement steps, out[2] refinements that fell back to a full eigensolve, out[3] eigensolves done block by block
 * (the x/y parity classes of a diatomic solved together, tf_eigh.hip.h: eigh_blocked), out[4] eigensolves where the matrix did not
 * have the block structure, or a block solve did not converge, and the full matrix was solved, out[5] full-matrix Jacobi solves that did
 * not converge in their sweep cap and were solved again by dsyevd.  A solve that fails on every path (non-finite input, dsyevd not
 * converging) is an error, TF_ELINALG. */
int tf_eigh_stats(tf_ctx *ctx, int64_t out[6]);

/* Fock builds of the native cycles on the packed layout since tf_create: out[0] builds that went over the shorter task list of a
 * class-diagonal density (no element between AOs of different x/y parity: every product of the skipped tasks is an exact zero,
 * J and K are bit for bit those of the full list), out[1] builds whose density was not and took the full list.  Builds through
 * tf_fock_jk / tf_fock_jk_device always take the full list (no test, no read-back). */
int tf_jk_path_stats(tf_ctx *ctx, int64_t out[2]);

/* HIP-event timing of the dominant kernel of the Fock build (the row pass over the stored tensor), recorded on
 * the stream each build is launched on.  enable: start (and reset) / stop collecting; read: synchronises the
 * recorded events, returns their summed duration and the number of launches, and resets. */
int tf_jk_profile(tf_ctx *ctx, int enable);
int tf_jk_profile_read(tf_ctx *ctx, double *seconds_total, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* TUNAFOCK_H */
