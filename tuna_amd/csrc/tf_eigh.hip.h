// tf_eigh.hip.h -- the symmetric eigensolver of the SCF code: the symmetry-blocked and the full solve (eigh), the warm-started
// eigenvector refinement of the cycles, orthogonaliser / diagonalise and the eigh_probe instrumentation.  Included by tf_scf.hip.h inside
// namespace tfscf, below Workspace, the TFS_* macros, gemm_rm, k_symmetrise and k_scale_cols, which it uses.  Its state is Workspace::eig
// (EigState); every buffer layout, the words of d_scal and of blk_ints come from tf_eigh_plan.h.  DESIGN.md 4.4b.

// one grow-only block of the eigensolver (as a hipError_t, for TFS_HIP); on refusal the slot is null
inline hipError_t eig_block(EigState &e, EigBlock slot, size_t bytes) { return (hipError_t)e.dev.ensure(slot, bytes); }

// ---- symmetry-blocked eigensolve ----------------------------------------------------------------------------------------------
// A diatomic on the z axis keeps the reflections x -> -x and y -> -y: every AO is even or odd under each (four classes, the same ones
// the packed tensor layout is blocked by), S, X = S^-1/2, the core Hamiltonian and a field along z do not connect different classes,
// and J, K of a class-diagonal density are class-diagonal again ((ij|kl) vanishes unless the four parities multiply to even,
// pyx:1324-1327).  The matrices the cycle diagonalises are then block diagonal after a permutation: at N = 400 blocks of
// 162 / 96 / 96 / 46 instead of 400, which rocsolver_dsyevd_strided_batched solves together in the time of the largest one
// (3.3 ms against 10.8 ms for the full matrix, `tools/gpu_eigh_blocks.py`).  Nothing is assumed: every call first measures the largest
// element that connects two classes (k_blk_cross) and declines -- the caller then solves the full matrix -- unless it is below
// 1e-14 of the largest element (a field along x, a symmetry-broken density or a basis without the structure end up there).
// Blocks are padded to the largest one with a decoupled diagonal JUST above the spectrum (1.01 x the Gershgorin bound: a padding value
// of n x max|a| -- 10^3 times the norm -- cost that factor in absolute accuracy, which the near-degenerate g/u pairs of a stretched
// diatomic cannot afford: 6e-7 in the core-guess orbital energies at N = 400); the eigenvalues of all blocks are ranked
// together (ties by block, then by position: a stable sort) and the vectors scattered back to the full basis.
inline void set_symmetry(Workspace &w, const std::vector<int> &cls) { if (cls != w.eig.sym_cls) { w.eig.sym_cls = cls; w.eig.sym_n = 0; } }

// out[0] = max |a_ij|, out[1] = max |a_ij| over pairs of different classes, out[2] = max_i sum_j |a_ij| (Gershgorin: no eigenvalue lies
// outside [-out[2], out[2]]); one workgroup per row.  Non-negative doubles order like their bit patterns (a NaN ends up above
// everything: declined).
__global__ void k_blk_cross(const double *__restrict__ A, const int *__restrict__ cls, int n, unsigned long long *__restrict__ out)
{
    __shared__ double sa[256], sx[256], ss[256];
    const int i = blockIdx.x, ci = cls[i];
    double all = 0.0, cross = 0.0, sum = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double v = fabs(A[(size_t)i * n + j]);
        all = fmax(all, v);
        sum += v;
        if (cls[j] != ci) cross = fmax(cross, v);
    }
    sa[threadIdx.x] = all; sx[threadIdx.x] = cross; ss[threadIdx.x] = sum;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
            sa[threadIdx.x] = fmax(sa[threadIdx.x], sa[threadIdx.x + st]); sx[threadIdx.x] = fmax(sx[threadIdx.x], sx[threadIdx.x + st]);
            ss[threadIdx.x] += ss[threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMax(out, (unsigned long long)__double_as_longlong(sa[0]));
        atomicMax(out + 1, (unsigned long long)__double_as_longlong(sx[0]));
        atomicMax(out + 2, (unsigned long long)__double_as_longlong(ss[0]));
    }
}

// B[b][r][c] = A[idx[b][r]][idx[b][c]] (symmetrised).  sizes == nullptr: every block padded to mmax x mmax with a decoupled diagonal `big`
// (rocSOLVER's batched solver wants one size); sizes given: compact blocks, leading dimension sizes[b] (the batched Jacobi kernel)
__global__ void k_blk_gather(const double *__restrict__ A, const int *__restrict__ idx, int n, int mmax, double big, double *__restrict__ B,
                             const int *__restrict__ sizes)
{
    const int b = blockIdx.y;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= mmax * mmax) return;
    const int r = e / mmax, c = e - r * mmax;
    const int i = idx[b * mmax + r], j = idx[b * mmax + c];
    if (sizes) {
        if (i >= 0 && j >= 0) B[(size_t)b * mmax * mmax + (size_t)r * sizes[b] + c] = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
        return;
    }
    double v;
    if (i >= 0 && j >= 0) v = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
    else v = (r == c) ? big : 0.0;
    B[((size_t)b * mmax + r) * mmax + c] = v;
}

// global ranks of the eigenvalues of all blocks (padding excluded): vals[rank] = value, src[rank] = b * mmax + t; single block of 1024
__global__ void k_blk_rank(const double *__restrict__ D, const int *__restrict__ idx, int nb, int mmax, double *__restrict__ vals, int *__restrict__ src)
{
    // member t of block b is real iff idx[b][t] >= 0 (members come first); the padded problems return their values ascending, so the
    // real ones are the first m_b of each block
    const int tot = nb * mmax;
    for (int q = threadIdx.x; q < tot; q += blockDim.x) {
        if (idx[q] < 0) continue;
        const double d = D[q];
        int rank = 0;
        for (int p = 0; p < tot; ++p) {
            if (idx[p] < 0) continue;
            const double dp = D[p];
            rank += (dp < d || (dp == d && p < q)) ? 1 : 0;
        }
        vals[rank] = d;
        src[rank] = q;
    }
}

// W[rank][:] = eigenvector `src[rank]` of its block, scattered to the full basis (zero outside the block); one workgroup per row
__global__ void k_blk_scatter(const double *__restrict__ B, const int *__restrict__ idx, const int *__restrict__ src, int n, int mmax,
                              double *__restrict__ W, const int *__restrict__ sizes)
{
    const int r = blockIdx.x;
    const int q = src[r], b = q / mmax, t = q - b * mmax;
    double *row = W + (size_t)r * n;
    for (int c = threadIdx.x; c < n; c += blockDim.x) row[c] = 0.0;
    __syncthreads();
    const double *v = B + (size_t)b * mmax * mmax + (size_t)t * (sizes ? sizes[b] : mmax);   // row t of the block in row-major terms = column t for rocSOLVER
    for (int c = threadIdx.x; c < mmax; c += blockDim.x) {
        const int i = idx[b * mmax + c];
        if (i >= 0) row[i] = v[c];
    }
}

// block of the eigenvector of global rank r
__global__ void k_blk_labels(const int *__restrict__ src, int mmax, int n, int *__restrict__ out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) out[r] = src[r] / mmax;
}

// acc[0] += 1 if any of the cnt status words is non-zero (a solver that did not converge); single thread
__global__ void k_info_fold(const int *__restrict__ info, int cnt, double *__restrict__ acc)
{
    int bad = 0;
    for (int i = 0; i < cnt; ++i) bad |= info[i] != 0;
    if (bad) acc[0] += 1.0;
}

// out = max |a| as the bits of a non-negative double (a NaN or an infinity compares above every finite value)
__global__ void k_amax_bits(const double *__restrict__ A, long long nn, unsigned long long *__restrict__ out)
{
    unsigned long long m = 0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nn; e += (long long)gridDim.x * blockDim.x)
        m = max(m, (unsigned long long)__double_as_longlong(fabs(A[e])));
    for (int d = 32; d > 0; d >>= 1) m = max(m, (unsigned long long)__shfl_xor((long long)m, d, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

// status words of the solve just queued: *bad = some solver did not converge.  Inside a cycle (eig_fail set) nothing is read here:
// the words are counted on the device and *bad stays false.
inline int solver_failed(Workspace &w, const rocblas_int *d_info, int cnt, bool *bad, std::string &msg)
{
    *bad = false;
    if (w.eig.eig_fail) { hipLaunchKernelGGL(k_info_fold, dim3(1), dim3(1), 0, TFS_ST, (const int *)d_info, cnt, w.eig.eig_fail); return TF_OK; }
    rocblas_int h[4] = {0, 0, 0, 0};
    TFS_HIP(tfs_memcpy(h, d_info, cnt * sizeof(rocblas_int), hipMemcpyDeviceToHost));
    for (int i = 0; i < cnt; ++i) *bad = *bad || h[i] != 0;
    return TF_OK;
}

// TF_OK: solved (W rows = eigenvectors, vals ascending).  TF_EINVAL with an empty msg: declined, the caller solves the full matrix
// (also when a block solve did not converge: W and vals are untouched until every block is known to be solved).
inline int eigh_blocked(Workspace &w, int n, double *W, double *vals, std::string &msg)
{
    static const bool off = getenv("TF_EIGH_BLOCKS") && getenv("TF_EIGH_BLOCKS")[0] == '0';
    static const int nmin = getenv("TF_EIGH_BLOCKS_NMIN") ? atoi(getenv("TF_EIGH_BLOCKS_NMIN")) : 40;   // below: one in-LDS Jacobi of the whole matrix is as fast
    EigState &eg = w.eig;
    if (off || (int)eg.sym_cls.size() != n || n < nmin) return TF_EINVAL;
    if (eg.sym_n != n) {                                           // tables for this class vector: whole, or none (sym_n = 0)
        SymPlan plan;
        if (!plan.build(eg.sym_cls)) return TF_EINVAL;
        eg.forget_tables();
        if (plan.lds_blocks()) TFS_HIP(eig_block(eg, EB_SYM_PREV, plan.blocks_len() * sizeof(double)));
        TFS_HIP(eig_block(eg, EB_SYM_IDX, plan.idx_len() * sizeof(int)));
        TFS_HIP(tfs_memcpy(eg.dev.p[EB_SYM_IDX], plan.idx.data(), plan.idx_len() * sizeof(int), hipMemcpyHostToDevice));
        TFS_HIP(eig_block(eg, EB_SYM_BUF, plan.buf_len() * sizeof(double)));
        TFS_HIP(eig_block(eg, EB_SYM_SRC, (size_t)n * sizeof(int)));
        eg.sym = plan;
        eg.sym_n = n;
    }
    const SymPlan &sp = eg.sym;
    const int nb = sp.nb, mmax = sp.mmax;
    if (!sp.worth_blocking()) return TF_EINVAL;                    // one class holds (nearly) everything: nothing to gain
    int *sym_idx = eg.dev.at<int>(EB_SYM_IDX), *sym_src = eg.dev.at<int>(EB_SYM_SRC);
    double *const sb = eg.dev.at<double>(EB_SYM_BUF), *const sym_prev = eg.dev.at<double>(EB_SYM_PREV);
    double *B = sb + sp.B(), *D = sb + sp.D(), *E = sb + sp.E();
    unsigned long long *flag = (unsigned long long *)(sb + sp.flag());
    const int *cls = sym_idx + sp.idx_cls();
    TFS_HIP(hipMemsetAsync(flag, 0, 3 * sizeof(double), TFS_ST));
    hipLaunchKernelGGL(k_blk_cross, dim3(n), dim3(256), 0, TFS_ST, W, cls, n, flag);
    double h[3];
    TFS_HIP(tfs_memcpy(h, flag, sizeof(h), hipMemcpyDeviceToHost));
    if (!(h[1] <= 1e-14 * h[0]) || !std::isfinite(h[0]) || !std::isfinite(h[2])) { ++eg.sym_declined; return TF_EINVAL; }
    const int g = (mmax * mmax + 255) / 256;
    const int *sizes = nullptr;
    if (sp.lds_blocks()) {
        // every block fits the in-LDS Jacobi kernel (tf_jacobi.hip.h): one launch, a workgroup per block, compact blocks, warm-started
        // from the block eigenvectors of the previous solve of the cycle (N2/cc-pVTZ: 60 = 26 + 14 + 14 + 6)
        static const bool no_warm = getenv("TF_EIGH_COLD") != nullptr;
        sizes = sym_idx + sp.idx_sizes();
        hipLaunchKernelGGL(k_blk_gather, dim3(g, nb), dim3(256), 0, TFS_ST, W, sym_idx, n, mmax, 0.0, B, sizes);
        const double *V0 = (eg.warm_ok && !no_warm && eg.sym_prev_n == n) ? sym_prev : nullptr;
        hipError_t e = hipSuccess;
        if (!tfjac::launch_batch(nb, mmax, sizes, B, (long long)mmax * mmax, D, mmax, (int *)w.d_info, TFS_ST, &e, V0, eg.warm_ok ? sym_prev : nullptr)) {
            msg = std::string("batched Jacobi eigensolver launch failed: ") + hipGetErrorString(e);
            return TF_ENODEVICE;
        }
        eg.sym_prev_n = eg.warm_ok ? n : 0;
    } else {
        hipLaunchKernelGGL(k_blk_gather, dim3(g, nb), dim3(256), 0, TFS_ST, W, sym_idx, n, mmax, 1.01 * h[2] + 1e-300, B, sizes);
        TFS_BLAS(rocsolver_dsyevd_strided_batched(w.blas, rocblas_evect_original, rocblas_fill_upper, mmax, B, mmax, (rocblas_stride)mmax * mmax,
                                                  D, mmax, E, mmax, w.d_info, nb));
    }
    bool bad = false;
    if (int rc = solver_failed(w, w.d_info, nb, &bad, msg)) return rc;
    if (bad) {                                                     // a block did not converge: forget its vectors, solve the full matrix
        eg.sym_prev_n = 0; eg.sv().blk_n = 0;
        ++eg.sym_declined;
        return TF_EINVAL;
    }
    hipLaunchKernelGGL(k_blk_rank, dim3(1), dim3(1024), 0, TFS_ST, D, sym_idx, nb, mmax, vals, sym_src);
    hipLaunchKernelGGL(k_blk_scatter, dim3(n), dim3(128), 0, TFS_ST, B, sym_idx, sym_src, n, mmax, W, sizes);
    ++eg.sym_solves;
    eg.sym_last_blocked = true;
    return TF_OK;
}

// Symmetric eigenproblem: W (in: symmetric matrix, out: row k = eigenvector k in row-major terms), vals ascending.
// n <= 64: single-launch in-LDS Jacobi (tf_jacobi.hip.h; measured 0.06/0.23/0.96 ms at n = 10/28/60 against 0.24/0.67/1.22 ms
// for dsyevd); larger: rocsolver_dsyevd (faster from n ~ 70 on).  TF_EIGH=rocsolver|jacobi overrides.
inline int eigh_route(Workspace &w, int n, double *W, double *vals, double *work_e, std::string &msg)
{
    static const bool force_rocsolver = getenv("TF_EIGH") && std::string(getenv("TF_EIGH")) == "rocsolver";
    static const bool force_jacobi = getenv("TF_EIGH") && std::string(getenv("TF_EIGH")) == "jacobi";
    static const int jac_nmax = getenv("TF_JACOBI_NMAX") ? std::min(TFJ_NMAX, std::max(2, atoi(getenv("TF_JACOBI_NMAX")))) : 64;
    EigState &eg = w.eig;
    eg.sym_last_blocked = false;
    if (!force_rocsolver && !force_jacobi) {                       // the symmetry blocks of a diatomic, solved together (declines if there are none)
        std::string bmsg;
        const int rb = eigh_blocked(w, n, W, vals, bmsg);
        if (rb == TF_OK) return TF_OK;
        if (!bmsg.empty()) { msg = bmsg; return rb; }
    }
    if (!force_rocsolver && n >= 2 && n <= (force_jacobi ? TFJ_NMAX : jac_nmax)) {
        const size_t bytes = (size_t)n * n * sizeof(double);
        TFS_HIP(eig_block(eg, EB_JAC_SCRATCH, bytes));
        if (eg.dev.cap[EB_JAC_PREV] < bytes) eg.jac_prev_n = 0;
        TFS_HIP(eig_block(eg, EB_JAC_PREV, bytes));
        double *jac_prev = eg.dev.at<double>(EB_JAC_PREV), *jac_in = nullptr;
        static const bool no_warm = getenv("TF_EIGH_COLD") != nullptr;
        const double *V0 = (eg.warm_ok && !no_warm && eg.jac_prev_n == n) ? jac_prev : nullptr;
        if (!eg.eig_fail) {                                        // checked at once: keep the matrix for dsyevd should the sweeps not converge
            TFS_HIP(eig_block(eg, EB_JAC_IN, bytes));
            jac_in = eg.dev.at<double>(EB_JAC_IN);
            TFS_HIP(hipMemcpyAsync(jac_in, W, bytes, hipMemcpyDeviceToDevice, TFS_ST));
        }
        hipError_t e = hipSuccess;
        if (tfjac::launch(n, W, vals, eg.dev.at<double>(EB_JAC_SCRATCH), (int *)w.d_info, TFS_ST, &e, V0, eg.warm_ok ? jac_prev : nullptr)) {
            bool bad = false;
            if (int rc = solver_failed(w, w.d_info, 1, &bad, msg)) return rc;
            if (!bad) {
                if (eg.warm_ok) eg.jac_prev_n = n;
                return TF_OK;
            }
            ++eg.jac_fallbacks;
            eg.jac_prev_n = 0;
            TFS_HIP(hipMemcpyAsync(W, jac_in, bytes, hipMemcpyDeviceToDevice, TFS_ST));
        } else if (e != hipSuccess) { msg = std::string("Jacobi eigensolver launch failed: ") + hipGetErrorString(e); return TF_ENODEVICE; }
    }
    TFS_BLAS(rocsolver_dsyevd(w.blas, rocblas_evect_original, rocblas_fill_upper, n, W, n, vals, work_e, w.d_info));
    bool bad = false;
    if (int rc = solver_failed(w, w.d_info, 1, &bad, msg)) return rc;
    if (bad) { msg = "Eigenvalues did not converge (rocsolver_dsyevd)"; return TF_ELINALG; }
    return TF_OK;
}

// x <- x 2^e (exact)
__global__ void k_ldexp(double *__restrict__ x, long long m, int e)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) x[i] = ldexp(x[i], e);
}

// eigh_route, and where the solve is checked at once (outside the iterations of a native cycle): a matrix with a NaN or an infinity is an
// error (np.linalg.eigh raises LinAlgError, scf:244), and one whose largest element lies outside [2^-100, 2^100] is solved at a power-of-two
// scale (exact; LAPACK's dsyev scales too, rocSOLVER's dsyevd does not: it returns wrong eigenvalues at 1e-100 and fails at 1e200).
inline int eigh(Workspace &w, int n, double *W, double *vals, double *work_e, std::string &msg)
{
    if (w.eig.eig_fail) return eigh_route(w, n, W, vals, work_e, msg);
    unsigned long long *am = (unsigned long long *)(w.d_scal + SC_AMAX);
    TFS_HIP(hipMemsetAsync(am, 0, sizeof(*am), TFS_ST));
    const int g = std::min(256, (n * n + 255) / 256);
    hipLaunchKernelGGL(k_amax_bits, dim3(g), dim3(256), 0, TFS_ST, W, (long long)n * n, am);
    unsigned long long hb = 0;
    TFS_HIP(tfs_memcpy(&hb, am, sizeof(hb), hipMemcpyDeviceToHost));
    if (hb >= 0x7ff0000000000000ULL) { w.eig.sym_last_blocked = false; msg = "eigensolver: the matrix has non-finite elements"; return TF_ELINALG; }
    double amax;
    std::memcpy(&amax, &hb, sizeof(amax));
    int ex = 0;
    if (amax > 0.0 && (amax < 0x1p-100 || amax > 0x1p100)) (void)std::frexp(amax, &ex);
    if (ex) hipLaunchKernelGGL(k_ldexp, dim3(g), dim3(256), 0, TFS_ST, W, (long long)n * n, -ex);
    const int rc = eigh_route(w, n, W, vals, work_e, msg);
    if (rc == TF_OK && ex) hipLaunchKernelGGL(k_ldexp, dim3(1), dim3(256), 0, TFS_ST, vals, (long long)n, ex);
    return rc;
}

// ---- warm-started eigenvector refinement ------------------------------------------------------------------------------------
// Inside an SCF cycle successive Fock matrices differ little, and what the cycle needs from a diagonalisation is the projector on
// the n_occ lowest eigenvectors (scf:183-211, 222-250).  Given the eigenvectors X of the previous solve, one step of the
// first-order refinement of Ogita & Aishima (Japan J. Indust. Appl. Math. 35 (2018) 1007), in the form used here:
//     X <- X (3/2 I - 1/2 X^T X)                     (Newton-Schulz: orthonormal to the square of the previous defect)
//     S = X^T A X,  lambda_i = s_ii,  e_ij = s_ij / (lambda_j - lambda_i),  X <- X + X E
// is five n^3 GEMMs on the matrix cores and converges quadratically.  Every occupied-virtual pair is rotated (its denominator is at
// least the gap); a pair inside the occupied or inside the virtual space is rotated only where that is well conditioned
// (|s_ij| <= 0.05 |lambda_j - lambda_i| and the difference above rounding level) -- the rotation inside a (near-)degenerate cluster
// does not change the projector, and diatomics are full of exact degeneracies (pi, delta, g/u pairs of separated atoms).
// Converged when the largest occupied-virtual rotation is below 1e-9.  No convergence in 16 steps, a rotation above 0.3 or a closed
// gap: the caller diagonalises (rocsolver_dsyevd) and restarts from those vectors.  At n = 400 a step costs ~0.15 ms against 9 ms
// for dsyevd (`tools/gpu_eigh_probe.py`); orbitals and orbital energies for the caller are produced once at the end of the cycle by a
// real eigensolve.  Storage: rows of Xr are the eigenvectors (Xr = X^T).

// lam[i] = s_ii, occupation weights w[i] (1 for the n_occ lowest), scal = {homo, lumo}; single block
__global__ void k_ref_diag(const double *__restrict__ S, int n, int n_occ, double *__restrict__ lam, double *__restrict__ wocc,
                           double *__restrict__ scal)
{
    __shared__ double s0[1024], s1[1024];
    for (int i = threadIdx.x; i < n; i += 1024) lam[i] = S[(size_t)i * n + i];
    __syncthreads();
    // ranks: the n_occ lowest values are occupied (ties broken by index, as a stable sort would)
    double homo = -1e300, lumo = 1e300;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double li = lam[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) { const double lj = lam[j]; rank += (lj < li || (lj == li && j < i)) ? 1 : 0; }
        const bool occ = rank < n_occ;
        wocc[i] = occ ? 1.0 : 0.0;
        if (occ) homo = fmax(homo, li); else lumo = fmin(lumo, li);
    }
    s0[threadIdx.x] = homo; s1[threadIdx.x] = lumo;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if (threadIdx.x < st) { s0[threadIdx.x] = fmax(s0[threadIdx.x], s0[threadIdx.x + st]); s1[threadIdx.x] = fmin(s1[threadIdx.x], s1[threadIdx.x + st]); }
        __syncthreads();
    }
    if (threadIdx.x == 0) { scal[0] = s0[0]; scal[1] = s1[0]; }
}

// E (row-major, antisymmetric) and per block: max |e_ij| over all pairs, and over the occupied-virtual pairs
// vcls (optional): block label of every vector (the exact solve they come from went block by block over the parity classes).  Vectors
// of different blocks are never rotated into each other: what couples them is rounding residue of the class-diagonal problem (the
// blocked solver dropped the same elements), and vectors that stay class-pure give densities with exact zeros between the classes,
// which the Fock build then exploits (tf_device.hip: the class-diagonal task list).  A coupling that is NOT residue (> 1e-6 as a rotation)
// is reported as a rotation of 1: the caller falls back to an exact solve, which will decline the blocks.
__global__ void k_ref_E(const double *__restrict__ S, const double *__restrict__ lam, const double *__restrict__ wocc, int n,
                        double *__restrict__ E, double *__restrict__ blockmax, const int *__restrict__ vcls)
{
    __shared__ double sm[256], so[256];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    double v = 0.0;
    bool ov = false, cross_bad = false;
    if (e < n * n) {
        const int i = e / n, j = e - i * n;
        if (i != j) {
            const double sij = 0.5 * (S[e] + S[(size_t)j * n + i]);
            const double dl = lam[j] - lam[i];
            ov = wocc[i] != wocc[j];
            if (ov || (fabs(sij) <= TF_REF_INTRA * fabs(dl) && fabs(dl) > TF_REF_CLUSTER)) v = sij / dl;
            if (vcls && vcls[i] != vcls[j]) {
                cross_bad = ov && fabs(v) > 1e-6;
                v = 0.0;
            }
        }
        E[e] = v;
    }
    sm[threadIdx.x] = cross_bad ? 1.0 : fabs(v); so[threadIdx.x] = cross_bad ? 1.0 : (ov ? fabs(v) : 0.0);
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) { sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + st]); so[threadIdx.x] = fmax(so[threadIdx.x], so[threadIdx.x + st]); }
        __syncthreads();
    }
    if (threadIdx.x == 0) { blockmax[2 * blockIdx.x] = sm[0]; blockmax[2 * blockIdx.x + 1] = so[0]; }
}

// out[i][:] = w[i] * X[i][:]
__global__ void k_scale_rows(const double *__restrict__ X, const double *__restrict__ w, double *__restrict__ out, int n)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n * n) out[e] = w[e / n] * X[e];
}

// the current spin's refinement block and the pinned read-back buffer, for n
inline int ref_ensure(Workspace &w, int n, std::string &msg)
{
    EigState &eg = w.eig;
    const RefLayout L(n);
    if (eg.dev.cap[eg.sv().ref_slot] < L.total() * sizeof(double)) eg.sv().ref_n = 0;
    TFS_HIP(eig_block(eg, (EigBlock)eg.sv().ref_slot, L.total() * sizeof(double)));
    TFS_HIP((hipError_t)eg.pin.ensure(0, L.npin() * sizeof(double)));
    if (!w.ev_pin) TFS_HIP(hipEventCreateWithFlags(&w.ev_pin, hipEventDisableTiming));
    return TF_OK;
}

// Refines the stored vectors against the symmetric A (device, row-major n x n).  TF_OK: *Xocc (a buffer of the workspace) holds the
// rows of the n_occ lowest eigenvectors (other rows zero).  TF_ELINALG: no convergence -- the caller diagonalises and calls ref_store.
inline int ref_refine(Workspace &w, int n, int n_occ, const double *A, double **Xocc, std::string &msg)
{
    EigState &eg = w.eig;
    SpinVectors &sv = eg.sv();
    double *const buf = eg.dev.at<double>(sv.ref_slot), *const h_pin = eg.pin.at<double>(0);
    if (sv.ref_n != n || !buf) return TF_ELINALG;
    static const bool dbg = getenv("TF_DEBUG") != nullptr;
    const RefLayout L(n);
    const size_t nn = L.nn;
    double *X = buf + L.X(), *Xn = buf + L.Xn(), *G = buf + L.G(), *Y = buf + L.Y(), *S = buf + L.S(), *E = buf + L.E();
    double *lam = buf + L.lam(), *wocc = buf + L.wocc(), *bmax = buf + L.bmax();
    const int g = (int)L.g;
    const int *vcls = (sv.vcls_n == n) ? reinterpret_cast<const int *>(buf + L.vcls()) : nullptr;
    // X <- (3/2 I - 1/2 G) X with G = X X^T (rows are the vectors)
    auto orthonormalise = [&]() -> int {
        TFS_BLAS(gemm_rm(w.blas, false, true, n, 1.0, X, X, 0.0, G));
        TFS_HIP(hipMemcpyAsync(Xn, X, nn * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
        TFS_BLAS(gemm_rm(w.blas, false, false, n, -0.5, G, X, 1.5, Xn));
        std::swap(X, Xn);
        return TF_OK;
    };
    ++eg.ref_solves;
    int rc = TF_OK;
    bool ok = false;
    // Every step ends with the update X <- X + E^T X and the orthonormalisation that either the next step or the end of the solve
    // needs; they are queued BEFORE the host looks at the step's convergence numbers (asynchronous copy to pinned memory + event), so
    // the read-back costs no idle time on the device.  (The stored vectors are orthonormal: no orthonormalisation before step 0.)
    const size_t npin = L.npin();
    if (!h_pin || eg.pin.cap[0] < npin * sizeof(double) || !w.ev_pin) return TF_ELINALG;
    for (int step = 0; step < 16 && !ok; ++step) {
        TFS_BLAS(gemm_rm(w.blas, false, false, n, 1.0, X, A, 0.0, Y));         // rows A x_i
        TFS_BLAS(gemm_rm(w.blas, false, true, n, 1.0, Y, X, 0.0, S));          // S = X^T A X
        hipLaunchKernelGGL(k_ref_diag, dim3(1), dim3(1024), 0, TFS_ST, S, n, n_occ, lam, wocc, buf + L.homo_lumo());
        hipLaunchKernelGGL(k_ref_E, dim3(g), dim3(256), 0, TFS_ST, S, lam, wocc, n, E, bmax, vcls);
        TFS_HIP(hipMemcpyAsync(h_pin, bmax, npin * sizeof(double), hipMemcpyDeviceToHost, TFS_ST));
        TFS_HIP(hipEventRecord(w.ev_pin, TFS_ST));
        TFS_HIP(hipMemcpyAsync(Xn, X, nn * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
        TFS_BLAS(gemm_rm(w.blas, true, false, n, 1.0, E, X, 1.0, Xn));         // X + E^T X   (rows)
        std::swap(X, Xn);
        if ((rc = orthonormalise())) return rc;
        TFS_HIP(hipEventSynchronize(w.ev_pin));
        const double *hb = h_pin;
        const double h[2] = {hb[2 * (size_t)g], hb[2 * (size_t)g + 1]};
        double emax = 0.0, eov = 0.0;
        for (int b = 0; b < g; ++b) { emax = std::max(emax, hb[2 * b]); eov = std::max(eov, hb[2 * b + 1]); }
        if (dbg) fprintf(stderr, "[tf refine] step %d: homo %.6f lumo %.6f max|E| %.3e max|E_ov| %.3e\n", step, h[0], h[1], emax, eov);
        if (!std::isfinite(emax) || !(h[1] > h[0]) || emax > 0.3) break;       // (the queued update is discarded with the vectors)
        eg.ref_steps += 1;
        ok = eov < 1e-9 && emax < 0.1;       // rotations inside the occupied or the virtual space leave the projector alone
    }
    if (ok) {
        if (X != buf + L.X()) {                                                // keep the vectors in the first slot for the next solve
            TFS_HIP(hipMemcpyAsync(buf + L.X(), X, nn * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
            X = buf + L.X();
        }
        double *Xw = buf + L.G();                                              // G's slot: free now
        hipLaunchKernelGGL(k_scale_rows, dim3(g), dim3(256), 0, TFS_ST, X, wocc, Xw, n);
        *Xocc = Xw;
        return TF_OK;
    }
    ++eg.ref_fallbacks;
    sv.ref_n = 0;
    return TF_ELINALG;
}

// n <= 64: the same refinement in one launch with every matrix in LDS (tf_refine.hip.h); one 8-byte status read per solve.
inline int ref_refine_lds(Workspace &w, int n, int n_occ, const double *A, double **Xocc, std::string &msg)
{
    EigState &eg = w.eig;
    SpinVectors &sv = eg.sv();
    double *const buf = eg.dev.at<double>(sv.ref_slot);
    if (sv.ref_n != n || !buf || n > TFR_NMAX) return TF_ELINALG;
    const RefLayout L(n);
    double *X = buf + L.X(), *Xw = buf + L.G(), *lam = buf + L.lam(), *wocc = buf + L.wocc();
    int *status = reinterpret_cast<int *>(w.d_scal + SC_REF_STATUS);
    hipError_t e = hipSuccess;
    ++eg.ref_solves;
    if (!tfref::launch(n, n_occ, A, X, lam, wocc, status, TFS_ST, &e)) {
        if (e != hipSuccess) { msg = std::string("refinement kernel launch failed: ") + hipGetErrorString(e); return TF_ENODEVICE; }
        return TF_ELINALG;
    }
    int h[2] = {0, 0};
    TFS_HIP(tfs_memcpy(h, status, 2 * sizeof(int), hipMemcpyDeviceToHost));
    static const bool dbg = getenv("TF_DEBUG") != nullptr;
    if (dbg) fprintf(stderr, "[tf refine/lds] n %d: %s after %d steps\n", n, h[0] ? "converged" : "NOT converged", h[1]);
    if (!h[0]) { ++eg.ref_fallbacks; sv.ref_n = 0; return TF_ELINALG; }
    eg.ref_steps += h[1];
    hipLaunchKernelGGL(k_scale_rows, dim3((int)L.g), dim3(256), 0, TFS_ST, X, wocc, Xw, n);
    *Xocc = Xw;
    return TF_OK;
}

// n <= 64, fused: A = sym(Xo^T Fao Xo), the refinement and the density P = occ * sym(C_occ C_occ^T) in the same launch
// (tf_refine.hip.h); nothing else of the "diagonalise and rebuild the density" step is left to launch.
inline int ref_density_lds(Workspace &w, int n, int n_occ, const double *Fao, const double *Xo, double *Pout, double occ, std::string &msg)
{
    EigState &eg = w.eig;
    SpinVectors &sv = eg.sv();
    double *const buf = eg.dev.at<double>(sv.ref_slot);
    if (sv.ref_n != n || !buf || n > TFR_NMAX) return TF_ELINALG;
    const RefLayout L(n);
    double *X = buf + L.X(), *lam = buf + L.lam(), *wocc = buf + L.wocc();
    int *status = reinterpret_cast<int *>(w.d_scal + SC_REF_STATUS);
    hipError_t e = hipSuccess;
    ++eg.ref_solves;
    if (!tfref::launch(n, n_occ, nullptr, X, lam, wocc, status, TFS_ST, &e, Fao, Xo, Pout, occ)) {
        if (e != hipSuccess) { msg = std::string("refinement kernel launch failed: ") + hipGetErrorString(e); return TF_ENODEVICE; }
        return TF_ELINALG;
    }
    int h[2] = {0, 0};
    TFS_HIP(tfs_memcpy(h, status, 2 * sizeof(int), hipMemcpyDeviceToHost));
    static const bool dbg = getenv("TF_DEBUG") != nullptr;
    if (dbg) fprintf(stderr, "[tf refine/lds fused] n %d: %s after %d steps\n", n, h[0] ? "converged" : "NOT converged", h[1]);
    if (!h[0]) { ++eg.ref_fallbacks; sv.ref_n = 0; return TF_ELINALG; }
    eg.ref_steps += h[1];
    return TF_OK;
}

// ---- refinement block by block (64 < n, every parity block <= 64 vectors: cc-pVQZ-size molecules) ---------------------------------
// The exact solves of such a matrix already run as one batched launch of the in-LDS Jacobi kernel over its blocks (eigh_blocked); the
// refinement does the same with the in-LDS refinement kernel (tf_refine.hip.h): a workgroup per block, its vectors and its block of A in
// LDS, the five products of a step on the matrix core -- one launch and one status read per solve instead of five rocBLAS GEMMs, two
// kernels and a read-back per STEP at the full dimension.  Each block keeps the number of occupied vectors the last exact solve gave it;
// after the launch the global aufbau order is verified (highest occupied value of all blocks below the lowest empty one), else -- or if
// a block did not converge, or A has an element between two classes -- the caller diagonalises.
__global__ void k_blk_noccs(const int *__restrict__ src, int mmax, int n_occ, int *__restrict__ noccs)
{
    __shared__ int cnt[4];
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int r = threadIdx.x; r < n_occ; r += blockDim.x) atomicAdd(&cnt[src[r] / mmax], 1);
    __syncthreads();
    if (threadIdx.x < 4) noccs[threadIdx.x] = cnt[threadIdx.x];
}

// combined[0] = 1 iff every block converged and the occupied values of all blocks lie below all empty ones; combined[1] = most steps
__global__ void k_blk_ref_finish(const int *__restrict__ sizes, const int *__restrict__ status, const double *__restrict__ lam,
                                 const double *__restrict__ wocc, int nb, int mmax, int *__restrict__ combined)
{
    __shared__ double sh[256], sl[256];
    double homo = -1e300, lumo = 1e300;
    for (int q = threadIdx.x; q < nb * mmax; q += 256) {
        const int b = q / mmax, t = q - b * mmax;
        if (t >= sizes[b]) continue;
        if (wocc[q] != 0.0) homo = fmax(homo, lam[q]); else lumo = fmin(lumo, lam[q]);
    }
    sh[threadIdx.x] = homo; sl[threadIdx.x] = lumo;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) { sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]); sl[threadIdx.x] = fmin(sl[threadIdx.x], sl[threadIdx.x + st]); }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int ok = (sh[0] < sl[0]) ? 1 : 0, steps = 0;
        for (int b = 0; b < nb; ++b) { ok = ok && status[2 * b]; steps = max(steps, status[2 * b + 1]); }
        combined[0] = ok; combined[1] = steps;
    }
}

// rows of the occupied vectors of all blocks in the full basis (block after block; the others zero): what ref_refine hands back
__global__ void k_blk_xocc(const double *__restrict__ Xb, const double *__restrict__ wocc, const int *__restrict__ idx, const int *__restrict__ sizes,
                           int n, int mmax, double *__restrict__ out)
{
    int r = blockIdx.x, b = 0;
    while (b < 3 && r >= sizes[b]) { r -= sizes[b]; ++b; }
    double *row = out + (size_t)blockIdx.x * n;
    for (int c = threadIdx.x; c < n; c += blockDim.x) row[c] = 0.0;
    __syncthreads();
    const double wv = wocc[b * mmax + r];
    if (wv == 0.0) return;
    const int m = sizes[b];
    const double *v = Xb + (size_t)b * mmax * mmax + (size_t)r * m;
    for (int c = threadIdx.x; c < m; c += blockDim.x) row[idx[b * mmax + c]] = wv * v[c];
}

inline int ref_refine_blocks(Workspace &w, int n, const double *A, double **Xocc, std::string &msg)
{
    EigState &eg = w.eig;
    SpinVectors &sv = eg.sv();
    const SymPlan &sp = eg.sym;
    double *const blk_X = eg.dev.at<double>(sv.blk_slot), *const ref_buf = eg.dev.at<double>(sv.ref_slot);
    if (sv.blk_n != n || !blk_X || eg.sym_n != n || sp.mmax > TFR_NMAX || !ref_buf) return TF_ELINALG;
    const int nb = sp.nb, mmax = sp.mmax;
    const int *sym_idx = eg.dev.at<int>(EB_SYM_IDX);
    double *const sb = eg.dev.at<double>(EB_SYM_BUF);
    double *B = sb + sp.B(), *D = sb + sp.D(), *E = sb + sp.E();
    unsigned long long *flag = (unsigned long long *)(sb + sp.flag());
    const int *cls = sym_idx + sp.idx_cls(), *sizes = sym_idx + sp.idx_sizes();
    int *blk_ints = eg.dev.at<int>(EB_BLK_INTS), *noccs = blk_ints + sv.nocc_off, *status = blk_ints + BI_STATUS, *combined = blk_ints + BI_COMBINED;
    ++eg.ref_solves; ++eg.blk_solves;
    TFS_HIP(hipMemsetAsync(flag, 0, 3 * sizeof(double), TFS_ST));
    hipLaunchKernelGGL(k_blk_cross, dim3(n), dim3(256), 0, TFS_ST, A, cls, n, flag);
    hipLaunchKernelGGL(k_blk_gather, dim3((mmax * mmax + 255) / 256, nb), dim3(256), 0, TFS_ST, A, sym_idx, n, mmax, 0.0, B, sizes);
    hipError_t e = hipSuccess;
    if (!tfref::launch_batch(nb, mmax, sizes, noccs, B, blk_X, (long long)mmax * mmax, D, E, mmax, status, TFS_ST, &e)) {
        if (e != hipSuccess) { msg = std::string("blocked refinement kernel launch failed: ") + hipGetErrorString(e); return TF_ENODEVICE; }
        return TF_ELINALG;
    }
    hipLaunchKernelGGL(k_blk_ref_finish, dim3(1), dim3(256), 0, TFS_ST, sizes, status, D, E, nb, mmax, combined);
    double *Xw = ref_buf + RefLayout(n).G();
    hipLaunchKernelGGL(k_blk_xocc, dim3(n), dim3(64), 0, TFS_ST, blk_X, E, sym_idx, sizes, n, mmax, Xw);
    int h[2] = {0, 0};
    double hf[3] = {0.0, 1.0, 0.0};
    TFS_HIP(tfs_memcpy(h, combined, sizeof(h), hipMemcpyDeviceToHost));
    TFS_HIP(tfs_memcpy(hf, flag, sizeof(hf), hipMemcpyDeviceToHost));
    static const bool dbg = getenv("TF_DEBUG") != nullptr;
    const bool diag_ok = std::isfinite(hf[0]) && hf[1] <= 1e-14 * hf[0];
    if (dbg) fprintf(stderr, "[tf refine/blocks] n %d (%d blocks <= %d): %s after %d steps%s\n", n, nb, mmax, h[0] ? "converged" : "NOT converged", h[1],
                     diag_ok ? "" : ", matrix not class-diagonal");
    if (!h[0] || !diag_ok) { ++eg.ref_fallbacks; ++eg.blk_fallbacks; sv.blk_n = 0; sv.ref_n = 0; return TF_ELINALG; }
    eg.ref_steps += h[1];
    *Xocc = Xw;
    return TF_OK;
}

// after a real eigensolve: rows of V (row-major, as eigh() leaves them) become the refinement start of the current spin
inline int ref_store(Workspace &w, int n, const double *V, std::string &msg, int n_occ = -1)
{
    int rc = ref_ensure(w, n, msg);
    if (rc) return rc;
    EigState &eg = w.eig;
    SpinVectors &sv = eg.sv();
    const SymPlan &sp = eg.sym;
    double *const buf = eg.dev.at<double>(sv.ref_slot);
    const int *sym_src = eg.dev.at<int>(EB_SYM_SRC);
    TFS_HIP(hipMemcpyAsync(buf, V, (size_t)n * n * sizeof(double), hipMemcpyDeviceToDevice, TFS_ST));
    sv.ref_n = n;
    sv.vcls_n = 0;
    if (eg.sym_last_blocked && eg.sym_n == n && sym_src) {         // V are the vectors of the blocked solve just done: keep their block labels
        int *vcls = reinterpret_cast<int *>(buf + RefLayout(n).vcls());
        hipLaunchKernelGGL(k_blk_labels, dim3((n + 255) / 256), dim3(256), 0, TFS_ST, sym_src, sp.mmax, n, vcls);
        sv.vcls_n = n;
    }
    // every block fits the in-LDS refinement kernel: keep the blocks' vectors (still in the solver's buffer) and their occupations
    static const bool blk_off = getenv("TF_REFINE_BLOCKS") && getenv("TF_REFINE_BLOCKS")[0] == '0';
    sv.blk_n = 0;
    if (!blk_off && n_occ > 0 && n > TFR_NMAX && eg.sym_last_blocked && eg.sym_n == n && sp.mmax <= TFR_NMAX && sym_src) {
        const size_t bytes = sp.blocks_len() * sizeof(double);
        TFS_HIP(eig_block(eg, (EigBlock)sv.blk_slot, bytes));
        TFS_HIP(eig_block(eg, EB_BLK_INTS, BI_LEN * sizeof(int)));
        TFS_HIP(hipMemcpyAsync(eg.dev.p[sv.blk_slot], eg.dev.at<double>(EB_SYM_BUF) + sp.B(), bytes, hipMemcpyDeviceToDevice, TFS_ST));
        hipLaunchKernelGGL(k_blk_noccs, dim3(1), dim3(64), 0, TFS_ST, sym_src, sp.mmax, n_occ, eg.dev.at<int>(EB_BLK_INTS) + sv.nocc_off);
        sv.blk_n = n;
    }
    return TF_OK;
}

// X = S^-1/2, S^-1, smallest eigenvalue (kernel:756-816).  The reference forms V sqrt(s) V^T and inverts it with
// LAPACK; here the inverse is applied in the eigenbasis, X = V s^-1/2 V^T, which is the same matrix.
inline int orthogonaliser_device(Workspace &w, int n, const double *dS, double *dX, double *dSinv, double *smallest, double *scratch,
                                 std::string &msg)
{
    const int nn = n * n, g = (nn + 255) / 256;
    double *W = scratch, *Vs = scratch + nn, *vals = scratch + 2 * (size_t)nn, *e = vals + n;
    hipLaunchKernelGGL(k_symmetrise, dim3(g), dim3(256), 0, TFS_ST, dS, W, n);
    int rc = eigh(w, n, W, vals, e, msg);
    if (rc) return rc;
    std::vector<double> hv(n);
    TFS_HIP(tfs_memcpy(hv.data(), vals, n * sizeof(double), hipMemcpyDeviceToHost));
    double mn = hv[0];
    for (double v : hv) mn = std::min(mn, v);
    if (smallest) *smallest = mn;
    if (mn < 0) { msg = "A negative overlap matrix eigenvalue was found!"; return TF_ELINALG; }
    // W holds V^T in row-major terms (row k = eigenvector k).  X = V f(s) V^T = (W^T diag) W
    // scale rows of W: Vs[k][i] = W[k][i] * f(s_k)  == scale "columns" of W^T
    for (int mode = 0; mode < 2; ++mode) {
        double *out = mode == 0 ? dX : dSinv;
        if (!out) continue;
        // Vs = diag(f(s)) W  -> use k_scale_cols on the transposed view: element e=(k,i) scaled by s[k]: need row scaling
        // row scaling = column scaling of the transpose; do it with a gemm-free kernel on W^T:
        // form Wt = W^T, scale columns, then X = Wt_scaled * W
        double one = 1.0, zero = 0.0;
        TFS_BLAS(rocblas_dgeam(w.blas, rocblas_operation_transpose, rocblas_operation_none, n, n, &one, W, n, &zero, W, n, Vs, n));
        hipLaunchKernelGGL(k_scale_cols, dim3(g), dim3(256), 0, TFS_ST, Vs, vals, mode, Vs, n);
        TFS_BLAS(gemm_rm(w.blas, false, false, n, 1.0, Vs, W, 0.0, out));
    }
    return TF_OK;
}

inline int orthogonaliser(Workspace &w, int n, const double *S, double *X, double *S_inv, double *smallest, std::string &msg)
{
    int rc = ensure(w, n, 6, msg);
    if (rc) return rc;
    const size_t nn = (size_t)n * n;
    double *dS = w.pool, *dX = dS + nn, *dSi = dX + nn, *scr = dSi + nn;
    TFS_HIP(tfs_memcpy(dS, S, nn * sizeof(double), hipMemcpyHostToDevice));
    rc = orthogonaliser_device(w, n, dS, dX, S_inv ? dSi : nullptr, smallest, scr, msg);
    if (rc) return rc;
    TFS_HIP(tfs_memcpy(X, dX, nn * sizeof(double), hipMemcpyDeviceToHost));
    if (S_inv) TFS_HIP(tfs_memcpy(S_inv, dSi, nn * sizeof(double), hipMemcpyDeviceToHost));
    return TF_OK;
}

// eps, C = eigh(sym(X^T F X)), C = X C'   (scf:222-250), host buffers
inline int diagonalise(Workspace &w, int n, const double *F, const double *X, double *eps, double *C, std::string &msg)
{
    int rc = ensure(w, n, 6, msg);
    if (rc) return rc;
    const size_t nn = (size_t)n * n;
    const int g = (int)((nn + 255) / 256);
    double *dF = w.pool, *dX = dF + nn, *t1 = dX + nn, *t2 = t1 + nn, *dW = t2 + nn, *vals = dW + nn, *e = vals + n;
    TFS_HIP(tfs_memcpy(dF, F, nn * sizeof(double), hipMemcpyHostToDevice));
    TFS_HIP(tfs_memcpy(dX, X, nn * sizeof(double), hipMemcpyHostToDevice));
    TFS_BLAS(gemm_rm(w.blas, true, false, n, 1.0, dX, dF, 0.0, t1));
    TFS_BLAS(gemm_rm(w.blas, false, false, n, 1.0, t1, dX, 0.0, t2));
    hipLaunchKernelGGL(k_symmetrise, dim3(g), dim3(256), 0, TFS_ST, t2, dW, n);
    rc = eigh(w, n, dW, vals, e, msg);
    if (rc) return rc;
    TFS_BLAS(gemm_rm(w.blas, false, true, n, 1.0, dX, dW, 0.0, t1));
    TFS_HIP(tfs_memcpy(eps, vals, n * sizeof(double), hipMemcpyDeviceToHost));
    TFS_HIP(tfs_memcpy(C, t1, nn * sizeof(double), hipMemcpyDeviceToHost));
    return TF_OK;
}

inline double *base_ifail(Workspace &w, int n) { return w.pool + 5 * (size_t)n * n; }

// Instrumentation: seconds per symmetric eigensolve of a random n x n matrix, variant 0 = dsyevd, 1 = dsyev, 2 = dsyevj.
// Status words: d_info has four (the batched variants 8, 9 write one per problem); dsyevdx / dsyevx leave theirs in d_scal + SC_PROBE_INFO
// (d_info holds their nev), and the n words of dsyevx's ifail lie in the pool behind the five matrices (base_ifail).
inline int eigh_probe(Workspace &w, int n, int variant, int reps, double *seconds, std::string &msg)
{
    int rc = ensure(w, n, 6, msg);
    if (rc) return rc;
    const size_t nn = (size_t)n * n;
    std::vector<double> h(nn);
    unsigned long long st = 88172645463325252ULL;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            st ^= st << 13; st ^= st >> 7; st ^= st << 17;
            double v = (double)(st % 2000001ULL) / 1e6 - 1.0;
            h[(size_t)i * n + j] = h[(size_t)j * n + i] = v;
        }
    double *A0 = w.pool, *A = A0 + nn, *V = A + nn, *vals = V + nn, *e = vals + n;
    TFS_HIP(tfs_memcpy(A0, h.data(), nn * sizeof(double), hipMemcpyHostToDevice));
    double tot = 0.0;
    for (int r = 0; r < reps + 1; ++r) {
        TFS_HIP(tfs_memcpy(A, A0, nn * sizeof(double), hipMemcpyDeviceToDevice));
        TFS_HIP(tfs_sync());
        auto t0 = std::chrono::steady_clock::now();
        if (variant == 0) TFS_BLAS(rocsolver_dsyevd(w.blas, rocblas_evect_original, rocblas_fill_upper, n, A, n, vals, e, w.d_info));
        else if (variant == 3) { int rc3 = eigh(w, n, A, vals, e, msg); if (rc3) return rc3; }
        else if (variant == 4 || variant == 5) {
            // partial spectrum: lowest 18 eigenpairs (the occupied orbitals of an Ar2-like SCF)
            rocblas_int *nev = w.d_info + 0;
            const int k = n < 18 ? n : 18;
            if (variant == 4)
                TFS_BLAS(rocsolver_dsyevdx(w.blas, rocblas_evect_original, rocblas_erange_index, rocblas_fill_upper, n, A, n, 0.0, 0.0, 1, k, nev,
                                           vals, V, n, (rocblas_int *)(w.d_scal + SC_PROBE_INFO)));
            else
                TFS_BLAS(rocsolver_dsyevx(w.blas, rocblas_evect_original, rocblas_erange_index, rocblas_fill_upper, n, A, n, 0.0, 0.0, 1, k, 0.0, nev,
                                          vals, V, n, (rocblas_int *)(base_ifail(w, n)), (rocblas_int *)(w.d_scal + SC_PROBE_INFO)));
        }
        else if (variant == 8 || variant == 9) {                  // a batch of four n x n problems in one call (the symmetry blocks of a diatomic)
            // pool: A0 | A | V | vals... : four matrices need 4 nn doubles from A on (ensure() gave 6 nn + vectors): copy A into 4 slots
            if (n > 256) { msg = "probe variant 8: n <= 256"; return TF_EINVAL; }
            if (n < 4) { msg = "probe variant 8: n >= 4"; return TF_EINVAL; }
            double *B = w.pool + nn;                              // 4 matrices of n x n behind A0 (A, V and the tail of the pool)
            for (int q = 1; q < 4; ++q) TFS_HIP(tfs_memcpy(B + q * nn, A0, nn * sizeof(double), hipMemcpyDeviceToDevice));
            double *vb = w.pool + 5 * nn, *eb = vb + 4 * n;       // 5 nn + 8 n doubles of the 6 nn + 4 n that ensure() gave: n >= 4; the four status words: d_info
            if (variant == 8)
                TFS_BLAS(rocsolver_dsyevd_strided_batched(w.blas, rocblas_evect_original, rocblas_fill_upper, n, B, n, (rocblas_stride)nn, vb, n, eb, n, w.d_info, 4));
            else
                TFS_BLAS(rocsolver_dsyevdj_strided_batched(w.blas, rocblas_evect_original, rocblas_fill_upper, n, B, n, (rocblas_stride)nn, vb, n, w.d_info, 4));
        }
        else if (variant == 6) TFS_BLAS(rocsolver_dsyevdj(w.blas, rocblas_evect_original, rocblas_fill_upper, n, A, n, vals, w.d_info));
        else if (variant == 7) {                                  // four n x n GEMMs: the cost of one eigenvector refinement step
            for (int q = 0; q < 4; ++q) TFS_BLAS(gemm_rm(w.blas, q & 1, false, n, 1.0, A0, A, 0.0, V));
        }
        else if (variant == 1) TFS_BLAS(rocsolver_dsyev(w.blas, rocblas_evect_original, rocblas_fill_upper, n, A, n, vals, e, w.d_info));
        else {
            double *resid = w.d_scal + SC_PROBE_RESID;
            rocblas_int *nsweeps = w.d_info;
            TFS_BLAS(rocsolver_dsyevj(w.blas, rocblas_esort_ascending, rocblas_evect_original, rocblas_fill_upper, n, A, n, 1e-14, resid, 100,
                                      nsweeps, vals, w.d_info));
        }
        TFS_HIP(tfs_sync());
        if (r > 0) tot += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    *seconds = tot / reps;
    return TF_OK;
}
