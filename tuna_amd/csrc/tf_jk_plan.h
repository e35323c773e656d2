// tf_jk_plan.h -- sizes, offsets and strides (in doubles) of the partial-sum buffers of the packed Fock build, stated ONCE: the allocation
// (jk_alloc_state) and the passes (jk_packed_pass, launch_jk_packed) of tf_jk_host.hip.h both take their numbers from here.  No HIP:
// tests/packed_model compiles it for the CPU, tests/test_jk_plan.py checks it against the formulas in NumPy.  DESIGN.md section 4.5b.
#pragma once
#include <algorithm>
#include <cstddef>

struct JkPlanIn {
    int N = 0, NW = 1, MP = 1, RS = 0;     // AOs; column chunks, parts of a walk, slots of a row part vector (the rows layout: 1, 1, 0)
    long long n_rows = 0, NPtot = 0;       // local tensor rows (0: a rank that owns none); padded pair index space
    // per table set t (0: one density per pass, groups of 8 rows; 1: two densities, groups of 4 rows)
    int n_groups[2] = {0, 0}, nseg[2] = {1, 1};
    long long ypart_len[2] = {0, 0};
};
// One pass over the tensor with ND = 1 or 2 densities.  Its partial arrays lie in the region of its pass type, as
// [column parts of density 0 | .. density 1 | row parts of density 0 | .. density 1].
struct JkPassPlan {
    size_t DI0 = 0, DJ0 = 0;               // region of this pass type in DI / DJ (general and class-diagonal buffers alike)
    size_t y0[2] = {0, 0};                 // ... in ypart: [0] general buffer (every pass overwrites what it reads: both types at 0),
                                           // [1] class-diagonal buffer (skipped slots must STAY zero: each pass type has its own region)
    size_t DIr = 0, DJr = 0;               // row parts behind the column parts, from the start of the region
    size_t sP = 0, sPp = 0, sy = 0, sJd = 0, sDIc = 0, sDIr = 0, sDJc = 0, sDJr = 0, sJt = 0;   // between the arrays of density 0 and 1
    size_t planeJd = 0, planeI = 0, planeJ = 0;   // between the column-part / Jd planes of the parts of a walk
};
enum { JK_CD_JROW = 0, JK_CD_YPART = 1, JK_CD_DI = 2, JK_CD_DJ = 3 };
struct JkPlan {
    size_t Jrow = 1, ypart = 1, DI = 1, DJ = 1, Jt = 1;   // the general buffers (Jrow: every layout)
    size_t cd[4] = {1, 1, 1, 1};                          // the class-diagonal set, by JK_CD_*
    JkPassPlan pass[2];                                   // [ND - 1]
};

static inline JkPlan jk_plan(const JkPlanIn &in)
{
    JkPlan P;
    const size_t N = (size_t)in.N, NW = (size_t)in.NW, MP = (size_t)in.MP, RS = (size_t)in.RS, npr = (size_t)in.NPtot;
    const size_t nrows = (size_t)std::max<long long>(1, in.n_rows), y[2] = {(size_t)in.ypart_len[0], (size_t)in.ypart_len[1]};
    const size_t ng[2] = {(size_t)std::max(1, in.n_groups[0]), (size_t)std::max(1, in.n_groups[1])};
    const size_t per_g = N * MP + RS;                     // column parts [MP][N] and the row part [RS] of one group / one row
    // everything sized for a two-density pass (the second density behind the first); DI, DJ: [one-density pass | two-density pass]
    P.Jrow = P.cd[JK_CD_JROW] = 2 * (size_t)std::max(1, std::max(1, in.NW) * in.MP) * nrows;
    P.ypart = std::max<size_t>(1, (size_t)std::max(in.ypart_len[0], 2 * in.ypart_len[1]));
    P.cd[JK_CD_YPART] = std::max<size_t>(1, y[0] + 2 * y[1]);
    P.DI = P.cd[JK_CD_DI] = (ng[0] + 2 * ng[1]) * per_g;
    P.DJ = P.cd[JK_CD_DJ] = 3 * nrows * per_g;
    P.Jt = 2 * (size_t)std::max(in.nseg[0], in.nseg[1]) * std::max<size_t>(1, npr);
    for (int t = 0; t < 2; ++t) {
        JkPassPlan &q = P.pass[t];
        q.planeJd = nrows * NW; q.planeI = ng[t] * N; q.planeJ = nrows * N;
        q.sP = N * N; q.sPp = npr; q.sy = y[t]; q.sJd = MP * q.planeJd; q.sJt = (size_t)in.nseg[t] * npr;
        q.sDIc = MP * q.planeI; q.sDIr = ng[t] * RS; q.sDJc = MP * q.planeJ; q.sDJr = nrows * RS;
        q.DI0 = t ? ng[0] * per_g : 0; q.DJ0 = t ? nrows * per_g : 0;
        q.y0[1] = t ? (size_t)std::max<long long>(0, in.ypart_len[0]) : 0;
        q.DIr = (t + 1) * q.sDIc; q.DJr = (t + 1) * q.sDJc;
    }
    return P;
}
