// tf_packed.h -- plain structs and constants of the parity-blocked packed tensor layout that host and device share (the layout is
// described at the top of tf_jkpacked.hip.h; the device views are in tf_layout.hip.h).  No HIP here: tf_packed_host.h builds the
// tables on the host from these, and tests/packed_model compiles both with g++.
#pragma once

#ifndef TF_SEG_PAD
#define TF_SEG_PAD 8             // segments start at multiples of this many doubles (even; 8 = 64 bytes, 16 = one 128-byte line)
#endif

struct KInfo { int offA, cnt; };  // segment of AO k in a row of class c: offset inside the section of k's class, stored values
struct TFInt2 { int x, y; };      // what the device reads as int2 (the upload sites assert the layout)

#define TF_JKP_JBB 8               // rows of a storage unit (and the largest row group)
#ifndef TF_JKP_VR1
#define TF_JKP_VR1 8               // rows of a group in a one-density pass: 8 (251 VGPRs, 2 waves per SIMD) or 4 (151 VGPRs, 3 waves per
                                   // SIMD, twice the steps: measured the same 2.1 ms at N = 400)
#endif
template <int ND> struct JKShape {           // virtual rows v = d * RB + r of a pass: RB tensor rows times ND densities
    static constexpr int VR = ND == 1 ? TF_JKP_VR1 : 8, RB = VR / ND;
};
#ifndef TF_JKP_GPW
#define TF_JKP_GPW 2               // row groups a wave works on at once: 2 (half waves on 64 columns) or 4 (quarter waves on 32 columns:
                                   // 20 % fewer wave steps at N = 400, but measured 8-15 % SLOWER -- DESIGN.md section 4.1)
#endif
#define TF_JKP_LG (64 / TF_JKP_GPW)   // lanes per group
#define TF_JKP_CW (2 * TF_JKP_LG)  // columns per chunk (2 per lane of a group's lanes)
#define TF_JKP_SEG 16            // segments of the super-group lists in the Jt reduction

struct JKGroup {
    int i, j0, nr, r0;           // rows r0..r0+nr-1 (local numbering) = pairs (i, j0..j0+nr-1), internal indices
    int c, lamj0;                // class of the rows; loc of j0
    int unr, p0;                 // rows of the storage unit that holds the group; position of the group's first row in it
    long long ub;                // base of the unit in the tensor
    int secoff[4];               // start of section a inside a row of this group
};
#ifndef TF_JKP_W
#define TF_JKP_W 4                // waves per workgroup (TF_JKP_GPW groups each): their Jt partials are merged in LDS before they are written
#endif
// up to 2 TF_JKP_W adjacent groups with the same i and class share one Jt partial (complete-row shape: NP[c] doubles at yoff)
struct JKSuper { int g0, ng, c, i; long long yoff; int ke[4]; };   // ke[a] = cntA[a][i]: the rows reach the members kappa < ke[a] of class a
struct JKTask { int super, w, part, pad; };   // part: which stretch of KS steps of the walk (the walks are cut for several ranks: shorter tasks)

#ifndef TF_JKR_THREADS
#define TF_JKR_THREADS 256         // (measured: 1024-thread blocks, 16 slices, are slower: 0.41 against 0.34 ms of tail at N = 400) threads of a jk_reduce_kernel block: 64 lanes x TF_JKR_THREADS / 64 slices of the rows / groups of an index
#endif
struct JKJtPlan { int sfirst[5]; int bfirst[5]; };   // supers of class c: sfirst[c] .. sfirst[c + 1]; blocks of class c: bfirst[c] .. bfirst[c + 1]

// Weight proxy of the shard plan (tf_shard_plan_pairs works from shell dimensions alone): the row lengths of the unblocked
// triangle, every triangle row rounded up to TF_TRI_PAD.  The blocked rows are ~1/4 of that, uniformly enough for balancing.
#ifndef TF_TRI_PAD
#define TF_TRI_PAD 16
#endif
inline long long tri_off(long long k)
{
    const long long q = k / TF_TRI_PAD, r = k % TF_TRI_PAD;     // sum over m = 1..k of m rounded up to the pad
    return TF_TRI_PAD * (TF_TRI_PAD * q * (q + 1) / 2 + r * (q + 1));
}
inline long long packed_row_len(long long i, long long j) { return (tri_off(i) + j + TF_TRI_PAD) & ~(long long)(TF_TRI_PAD - 1); }
