// tf_dbasis.hip.h -- device view of the basis (shells, shell pairs, per-pair tables) shared by the translation units that hold
// ERI kernels (tf_device.hip and tf_eri_team.hip).  Its plain records DShell and DPair are in tf_eri_types.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "tf_internal.h"
#include "tf_layout.hip.h"
#include "tf_eri_types.h"

namespace tfk {

struct DBasis {
    const DShell *shells;
    const DPair *pairs;
    const int8_t *c_lx, *c_ly, *c_lz;
    const double *c_scale;
    const double *pp_p, *pp_Pz, *pp_K;
    const double *epool;
    const double *boys;      // [NGRID][NORD]
    // per-L Cartesian->spherical rows (CSR over the components of one shell): row base sphL_base[L], then ptr/idx/val
    const int *sphL_base, *sphL_ptr, *sphL_idx;
    const double *sphL_val;
    // per shell pair, entry f = ca * ncb + cb (DPair::tab_off): index word ((ax (Lb+1) + bx) | (ay (Lb+1) + by) << 8 | (az (Lb+1) + bz)
    // << 16 | x parity << 24 | y parity << 25), normalisation ratio, position word (ca << 8 | cb), parity-class order
    const int *ct_ix, *ct_pos, *ct_ord;
    const double *ct_sc;
    const LRec *lrec;
    const unsigned short *tup;
    // packed layout (set by tf_build_eri): the layout tables and the stride of a slab row (complete-row shape, max_c NP[c] doubles)
    BLayout bl;
    long long RLS;
    // team kernels (tf_eri_team.hip.h; set by tf_build_eri): per ket pair the slab offsets of its output pairs (kq_off[kq_ptr[pair] + kappa],
    // -1: not stored), per pair class the Cartesian -> output transform of its component pairs, parity class by parity class
    const int *kq_ptr, *kq_off, *kt_ptr, *kt_k;
    const double *kt_c;
    const int *tflat;            // flat component / output lists of the class pairs (TClass::flat_off)
};

}  // namespace tfk
