// tf_triples.hip.h -- the non-iterative triples of CCSD(T), QCISD(T) and full MP4 for a closed shell (calculate_restricted_CCSD_T_energy,
// tuna_cc.py:2688-2758; the triples of run_restricted_MP4, tuna_mp.py:403-428 and :1605-1637).  Chemists' integrals, occupied i, j, k, m
// (o orbitals), virtual a, b, c, f (v orbitals):
//     X_ijk^abc = sum_f (ia|bf) t2[k,j,c,f] - sum_m (ia|jm) t2[m,k,b,c]
//     W_ijk^abc = the sum over the six simultaneous permutations of the columns (i a), (j b), (k c) of X
//     V_ijk^abc = s [(jb|kc) t1[i,a] + (ia|kc) t1[j,b] + (ia|jb) t1[k,c]]         s = 1 (CCSD(T)), 2 (QCISD(T)), V = 0 (MP4)
//     D_ijk^abc = e_i + e_j + e_k - e_a - e_b - e_c
//     e_ijk     = 1/3 sum_abc (W + V)^abc (4 W^abc + W^bca + W^cab - 2 W^cba - 2 W^acb - 2 W^bac) / D      (all W at the same ijk)
//     E_T       = the sum of e_ijk over ALL ordered (i, j, k)
// The last bracket is the average over the six orderings of (i, j, k) of the reference's (4, 1, 1, -4, -1, -1) form, so e_ijk is
// symmetric in (i, j, k) and an unordered triple i >= j >= k counts once with the number of its distinct orderings.
//
// The caller (tf_triples_rhf) writes, per unordered triple, the six X_pqr = [a][b][c] of the orderings (p, q, r) of (i, j, k) with rocBLAS;
// buffer number n holds the ordering (o_P[n][0], o_P[n][1], o_P[n][2]) of o = (i, j, k), P[n][m] = perm3(n, m) below.  With v = (a, b, c),
//     W^abc = sum_n X_n[v_P[n][0]][v_P[n][1]][v_P[n][2]].
// triples_energy_kernel: one workgroup per unordered triple {t0 <= t1 <= t2} of virtual-index tiles of TT^3 elements.  Slot s of its LDS image
// is W at the tile position (t_P[s][0], t_P[s][1], t_P[s][2]); the six slots are closed under every permutation above: buffer n at the tile
// position u = s o n (u[m] = s[n[m]]), local element (l_n[0], l_n[1], l_n[2]), is what slot s, local l, needs of it.  The kernel reads the 36
// (buffer, position) tiles along c (one pass per buffer, a barrier between passes: within a pass (u, x, y, z) -> (s, l) is one-to-one, so
// no two threads touch one LDS word), then sums (W + V) Y / D over the DISTINCT positions of the six (t0 = t1 or t1 = t2 make slots
// coincide: the copies are filled alike and only the first is summed).  Elements beyond v are read as zeros and not summed.  W never
// reaches HBM and every X element is read once (per copy of a coincident slot).  LDS image: 6 slots of TT (TT (TT + 1) + 1) doubles,
// strides (TT (TT + 1) + 1, TT + 1, 1) -- all odd, so the transposed accesses of a pass (8 consecutive z onto any of the three local
// indices) fall on distinct banks: 28 032 bytes at TT = 8, plus the reduction's 4 KB.
#pragma once
#include <hip/hip_runtime.h>

namespace tftriples {

constexpr int TT = 8;                                    // cubic tile of virtual indices
constexpr int TT3 = TT * TT * TT;
constexpr int S1 = TT + 1, S0 = TT * S1 + 1, SLOT = TT * S0;
constexpr int THREADS = 256;

// The six permutations of (0, 1, 2) in lexicographic order, entry m of number n: {0,1,2} {0,2,1} {1,0,2} {1,2,0} {2,0,1} {2,1,0}.  Arithmetic,
// not a table: with the loops below unrolled every use folds to a constant (a table in memory put a dependent load in front of every
// tensor load)
__host__ __device__ constexpr int perm3(int n, int m)
{
    const int p0 = n >> 1, r0 = p0 == 0 ? 1 : 0, r1 = p0 == 2 ? 1 : 2;
    return m == 0 ? p0 : ((m == 1) == ((n & 1) == 0) ? r0 : r1);
}
__host__ __device__ constexpr int perm_index(int p0, int p1, int p2) { return 2 * p0 + (p1 > p2 ? 1 : 0); }
__device__ __forceinline__ int pick(int m, int x0, int x1, int x2) { return m == 0 ? x0 : (m == 1 ? x1 : x2); }
static_assert(perm3(1, 1) == 2 && perm3(1, 2) == 1 && perm3(3, 0) == 1 && perm3(3, 1) == 2 && perm3(3, 2) == 0 && perm3(4, 1) == 0 &&
              perm3(4, 2) == 1 && perm3(5, 1) == 1 && perm3(5, 2) == 0 && perm_index(perm3(4, 0), perm3(4, 1), perm3(4, 2)) == 4, "perm3");

struct EnergyArgs {
    const double *X[6];          // the six X_pqr, [v][v][v] each
    const int *tiles;            // [n_blocks][3]: t0 <= t1 <= t2
    const double *g1;            // (ia|jb) as [i][a][j][b]
    const double *t1;            // [o][v]; not read when vscale == 0
    const double *eps;           // [N]
    double vscale;               // 1 (CCSD(T)), 2 (QCISD(T)), 0 (MP4: V = 0)
    int i, j, k;                 // the triple, counted from the first active occupied orbital
    int n_frozen, n_occ, o, v;
    double *partial;             // [n_blocks][2]: connected, disconnected (without the factor 1/3)
};

constexpr int PER_THREAD = 6 * TT3 / THREADS;            // elements of the six positions per thread: 12
static_assert(THREADS == 256 && TT == 8 && PER_THREAD == 12, "the element numbering below: e = tid + 256 it, position it / 2");

__global__ __launch_bounds__(THREADS) void triples_energy_kernel(EnergyArgs A)
{
    __shared__ double W[6 * SLOT];
    __shared__ double red[2 * THREADS];
    const int tid = threadIdx.x, v = A.v;
    const int t0 = A.tiles[3 * blockIdx.x], t1 = A.tiles[3 * blockIdx.x + 1], t2 = A.tiles[3 * blockIdx.x + 2];
    // element e = tid + 256 it of the 6 x 8^3: tile position u = it / 2 (the same for the whole workgroup), local (x, y, z) with z fastest
    const int xl = tid >> 6, y = (tid >> 3) & 7, z = tid & 7;
    // ---- W at the six positions: one pass per buffer, its twelve loads in flight together
#pragma unroll
    for (int n = 0; n < 6; ++n) {
        const int n0 = perm3(n, 0), n1 = perm3(n, 1), n2 = perm3(n, 2);
        const double *__restrict__ X = A.X[n];
        double val[PER_THREAD];
#pragma unroll
        for (int it = 0; it < PER_THREAD; ++it) {
            const int u = it >> 1, x = xl + 4 * (it & 1);
            const int gx = pick(perm3(u, 0), t0, t1, t2) * TT + x, gy = pick(perm3(u, 1), t0, t1, t2) * TT + y, gz = pick(perm3(u, 2), t0, t1, t2) * TT + z;
            val[it] = (gx < v && gy < v && gz < v) ? X[((size_t)gx * v + gy) * v + gz] : 0.0;
        }
#pragma unroll
        for (int it = 0; it < PER_THREAD; ++it) {
            const int u = it >> 1, x = xl + 4 * (it & 1);
            const int u0 = perm3(u, 0), u1 = perm3(u, 1), u2 = perm3(u, 2);
            // s[n[m]] = u[m], l[n[m]] = (x, y, z)[m]
            int s0 = 0, s1 = 0, s2 = 0, l0 = 0, l1 = 0, l2 = 0;
            if (n0 == 0) { s0 = u0; l0 = x; } else if (n0 == 1) { s1 = u0; l1 = x; } else { s2 = u0; l2 = x; }
            if (n1 == 0) { s0 = u1; l0 = y; } else if (n1 == 1) { s1 = u1; l1 = y; } else { s2 = u1; l2 = y; }
            if (n2 == 0) { s0 = u2; l0 = z; } else if (n2 == 1) { s1 = u2; l1 = z; } else { s2 = u2; l2 = z; }
            const int at = perm_index(s0, s1, s2) * SLOT + l0 * S0 + l1 * S1 + l2;
            if (n == 0) W[at] = val[it]; else W[at] += val[it];
        }
        __syncthreads();
    }
    // ---- the energy over the distinct positions
    const double eo = A.eps[A.n_frozen + A.i] + A.eps[A.n_frozen + A.j] + A.eps[A.n_frozen + A.k];
    const int o = A.o;
    double conn = 0.0, disc = 0.0;
#pragma unroll
    for (int it = 0; it < PER_THREAD; ++it) {
        const int s = it >> 1, l0 = xl + 4 * (it & 1), l1 = y, l2 = z;
        const int q0 = perm3(s, 0), q1 = perm3(s, 1), q2 = perm3(s, 2);
        const int ta = pick(q0, t0, t1, t2), tb = pick(q1, t0, t1, t2), tc = pick(q2, t0, t1, t2);
        bool dup = false;                                 // an earlier slot at the same tile position
#pragma unroll
        for (int p = 0; p < s; ++p)
            dup = dup || (pick(perm3(p, 0), t0, t1, t2) == ta && pick(perm3(p, 1), t0, t1, t2) == tb && pick(perm3(p, 2), t0, t1, t2) == tc);
        const int a = ta * TT + l0, b = tb * TT + l1, c = tc * TT + l2;
        if (dup || a >= v || b >= v || c >= v) continue;
        // W at the permutation pi of (a, b, c): slot s o pi, local (l_pi[0], l_pi[1], l_pi[2])
        auto wp = [&](int p0, int p1, int p2) {
            return W[perm_index(pick(p0, q0, q1, q2), pick(p1, q0, q1, q2), pick(p2, q0, q1, q2)) * SLOT + pick(p0, l0, l1, l2) * S0 +
                     pick(p1, l0, l1, l2) * S1 + pick(p2, l0, l1, l2)];
        };
        const double w = wp(0, 1, 2);
        // 4 W^abc + W^bca + W^cab - 2 W^cba - 2 W^acb - 2 W^bac as four differences: exactly 0 where a = b = c (v = 1: E_T is exactly 0.0)
        const double wbac = wp(1, 0, 2);
        const double yv = 2.0 * (w - wp(2, 1, 0)) + 2.0 * (w - wp(0, 2, 1)) + (wp(1, 2, 0) - wbac) + (wp(2, 0, 1) - wbac);
        const double D = eo - A.eps[A.n_occ + a] - A.eps[A.n_occ + b] - A.eps[A.n_occ + c];
        const double yd = yv / D;
        conn += w * yd;
        if (A.vscale != 0.0) {
            const size_t ia = (size_t)A.i * v + a, jb = (size_t)A.j * v + b, kc = (size_t)A.k * v + c;
            const size_t row = (size_t)o * v;
            const double V = A.vscale * (A.g1[jb * row + kc] * A.t1[ia] + A.g1[ia * row + kc] * A.t1[jb] + A.g1[ia * row + jb] * A.t1[kc]);
            disc += V * yd;
        }
    }
    red[tid] = conn; red[THREADS + tid] = disc;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) { red[tid] += red[tid + h]; red[THREADS + tid] += red[THREADS + tid + h]; }
        __syncthreads();
    }
    if (tid == 0) { A.partial[2 * (size_t)blockIdx.x] = red[0]; A.partial[2 * (size_t)blockIdx.x + 1] = red[THREADS]; }
}

// out[0..1] = the sums of partial[block][0..1] in block order with a fixed association: thread t sums the blocks
// [t chunk, (t + 1) chunk) in order, thread 0 then sums the 256 chunk sums in order.  One workgroup.
__global__ __launch_bounds__(THREADS) void triples_sum_partials_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ out)
{
    __shared__ double red[2 * THREADS];
    const int tid = threadIdx.x, chunk = (nblk + THREADS - 1) / THREADS;
    double c = 0.0, d = 0.0;
    for (int b = tid * chunk; b < nblk && b < (tid + 1) * chunk; ++b) { c += partial[2 * (size_t)b]; d += partial[2 * (size_t)b + 1]; }
    red[tid] = c; red[THREADS + tid] = d;
    __syncthreads();
    if (tid == 0) {
        double sc = 0.0, sd = 0.0;
        for (int t = 0; t < THREADS; ++t) { sc += red[t]; sd += red[THREADS + t]; }
        out[0] = sc; out[1] = sd;
    }
}

// MP4's amplitudes: t2[i][j][a][b] = (ia|jb) / (e_i + e_j - e_a - e_b) from g1 = [i][a][j][b]
__global__ void triples_mp2_amplitudes_kernel(const double *__restrict__ g1, const double *__restrict__ eps, int n_frozen, int n_occ, int o, int v,
                                              double *__restrict__ t2)
{
    const long long total = (long long)o * o * v * v;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        long long r = e;
        const int b = (int)(r % v); r /= v;
        const int a = (int)(r % v); r /= v;
        const int j = (int)(r % o);
        const int i = (int)(r / o);
        const double D = (eps[n_frozen + i] + eps[n_frozen + j]) - (eps[n_occ + a] + eps[n_occ + b]);
        t2[e] = g1[(((long long)i * v + a) * o + j) * v + b] / D;
    }
}

}  // namespace tftriples
