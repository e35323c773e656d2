// tf_eri_types.h -- plain launch records and constants of the ERI kernels that host and device share.  No HIP here: tf_eri_plan.h fills
// the records on the host from integers, the kernel headers (tf_eri.hip.h, tf_eri_team.hip.h, tf_dbasis.hip.h) read them, and
// tests/packed_model compiles both with g++.
#pragma once
#include <vector>

#define TF_ERI_THREADS 256
#define TF_BLK_DOUBLES 1024   // LDS doubles of the Cartesian (cc,cd) sub-block buffer of the fused ket transform
// LDS copy of the Cartesian->spherical rows of shell types C and D (the global CSR is a chain of dependent L2 loads per output)
#define TF_CSR_CAP 144                                     // entries per shell type (h shells: 11 rows)
#define TF_CSR_DOUBLES (2 * TF_CSR_CAP + (2 * TF_CSR_CAP + 32) / 2)
#define TF_TEAM_LMAX 6           // pair sums La + Lb, Lc + Ld the team kernels are instantiated for (up to two f shells)
#define TF_CF_KMAX 2

namespace tfk {

// ---- the basis as the kernels read it: one record per shell and per shell pair A >= B (DBasis, tf_dbasis.hip.h, points at arrays of them)
struct DShell { int L, ncomp, comp_off, cart_off; };
struct DPair {
    int A, B, La, Lb, npp, pp_off, nE, cls;
    long long e_off;
    int nca, ncb, compoff_a, compoff_b, cartoff_a, cartoff_b;
    int outoff_a, outoff_b;      // first OUTPUT AO (spherical, or Cartesian for CARTHARM) of the two shells; set by tf_build_eri
    int tab_off;                 // component-pair tables of this pair in DBasis::ct_* (nca * ncb entries)
    int pcls[5];                 // ct_ord: component pairs ordered by (x, y) parity class; class c is [pcls[c], pcls[c + 1])
};

// Every host table of the device basis that follows from a tf::Basis alone (tf::build_device_tables, tf_host.cpp): tf_set_basis uploads
// them and keeps pair_class, class_pairs, hp and the ct_* mirrors for the tensor build.
struct DeviceTables {
    std::vector<DShell> hs;
    std::vector<DPair> hp;                        // with cls, tab_off and pcls; the output offsets stay 0 (tf_build_eri)
    std::vector<int> pair_class;                  // class id of every shell pair: same angular momenta, component counts, components, contraction depth class
    std::vector<std::vector<int>> class_pairs;    // pairs of each class, ascending
    // component-pair tables of every shell pair (eri_cfact_kernel): index word, position, parity-class order, normalisation ratio
    std::vector<int> ct_ix, ct_pos, ct_ord;
    std::vector<double> ct_sc;
    // per-L spherical rows as CSR over the Cartesian components of one shell
    std::vector<int> sph_base, sph_ptr, sph_idx;
    std::vector<double> sph_val;
};

struct QClass {
    int La, Lb, Lc, Ld, L, tsize;
    int nca, ncb, ncc, ncd, ncomp;
    int npp_ab, npp_cd, npq;   // maxima over the launch (LDS capacity); the actual depths come from the pair records
    int nEab, nEcd;
    int PB, stride;        // primitive quartets per LDS batch, LDS column stride of the R tables
    int G, ncp;            // multi kernel: shell quartets per workgroup, padded components per quartet
    int n_ket;             // ket pairs in this launch
    int fused, spherical, nsc, nsd, Nout, ld, offBlk;   // fused ket transform: output dims of shells C, D; T2 geometry; LDS block buffer
    int offG;              // factorised kernel: ket half of the z tables, (Lc+1)(Ld+1)(La+Lb+1) nM doubles
    int offTab;            // factorised kernel: per-pair component tables, (nab + ncc*ncd) * 2 doubles (scale, two offset words)
    int offCsr;            // fused spherical ket transform: LDS copy of the two shells' Cartesian->spherical CSR rows (TF_CSR_DOUBLES)
    int tri;               // packed layout: only kets with first shell <= the bra's first shell are needed ((kl) <= (ij))
    int tupG_off, tupXZ_off;   // factorised kernel: index words of its table entries in DBasis::tup (LRec of the class)
    // LDS carve-out, offsets in doubles
    int offR, offPref, offPQ, offRed, offEab, offEcd, offScale, offLmn, lds_doubles;
};

struct CFCaps {
    int offR, capR, offPref, offPQ, offPP, offG, capG, offX, offZ, capXZ, offTupG, offTupXZ, offEab, capEab, offEcd, capEcd;
    int offRed, lds_doubles, tri;
    int gtab_doubles;                // GTAB launches: offG / offX / offZ are relative to the workgroup's block of this many doubles in global memory
    int dbg_npq_lo, dbg_npq_hi;      // profiling aid (TF_ERI_DBG_NPQ=lo:hi): only quartets with lo <= primitive quartets <= hi are computed
    int offKm, capKm;                // FAMILY launches: weights of the members' primitive pairs, [member][primitive pair] (capKm doubles)
    int team_lmax, team_pqmax;       // quartets with both pair sums <= team_lmax and <= team_pqmax primitive quartets belong to eri_teamc_kernel (-1: none)
};

// What a shell quartet with the angular momenta (La, Lb | Lc, Ld) needs to know, tabulated once per tf_build_eri (index
// ((La * 6 + Lb) * 6 + Lc) * 6 + Ld): sizes of the per-axis factor tables of eri_cfact_kernel, the index words of their entries
// (DBasis::tup) and the primitive quartets per batch the launch of its shell-pair groups has LDS for.
struct LRec { int L, nM, tsize, nT, xz, gsz, lgG, lgX, nb_cap, tupG_off, tupXZ_off, pad; };

struct TClass {
    int La, Lb, Lc, Ld;
    int nTab, nTcd, nT;           // exponent tuples of one axis: (La+1)(Lb+1), (Lc+1)(Ld+1), their product
    float inv_nTcd;
    int nab, ncd;                 // Cartesian component pairs of the bra / ket shell pair
    int pA[5], pK[5], pS[5];      // parity-class offsets: bra component pairs, ket component pairs, ket output pairs (class-sorted lists)
    int nkap, nnzT;               // ket output pairs; entries of the ket pair transform
    int tabA, tabK;               // DBasis::ct_* offsets of a representative bra / ket pair (the tables are the same for a whole class)
    int ktp_off, kte_off;         // ket pair transform of the ket class: row pointers at kt_ptr[ktp_off ..], entries at kt_k / kt_c[kte_off ..]
    int n_ket;                    // ket pairs of the launch (class list prefix)
    int nEab, nEcd;               // doubles of one Hermite table of the bra / ket pair
    int vcap;                     // doubles of a team's component block (eri_teamc_kernel: of its table scratch)
    int nacc;                     // parity-allowed Cartesian components of a quartet (eri_teamc_kernel: the accumulation block)
    int oE12, oOffA, oScA, oOffK, oTp, oTk, oTc, shared_doubles, team_doubles;   // LDS carve-out, in doubles
    // flat component / output lists (classes whose parity-allowed components fit the team's block: one loop over all of them instead
    // of one per parity class): DBasis::tflat[flat_off ..] = nacc words (bra index | ket index << 16, class-sorted indices), then nout
    // pairs (bra index | output pair << 16, offset of the bra row inside the block)
    int flat, flat_off, nflat, nout, oCompW, oOutW, oRowOff;   // nflat: words to stage (components padded to an even count, then outputs)
    float invK[4], invS[4];       // 1 / (ket component pairs of class c), 1 / (ket output pairs of class c)
    long long RLS;                // stride of a slab row
};

}  // namespace tfk

namespace tf {
struct Basis;
// exact_class: pairs of different contraction depth never share a class (TF_ERI_EXACT_CLASS, read by the caller)
void build_device_tables(const Basis &bs, bool exact_class, tfk::DeviceTables &out);
}  // namespace tf
