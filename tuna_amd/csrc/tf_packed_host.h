// tf_packed_host.h -- host tables of the parity-blocked packed tensor layout (tf_packed.h, tf_layout.hip.h, tf_jkpacked.hip.h): layout
// tables, row tables and storage units, work tables of the Fock kernel, tables of the tensor's consumers.  Pure C++ (no HIP, no
// environment, no context): compiled into libtunafock (tf_device.hip uploads what these builders make) and into the CPU test library
// of tests/packed_model.  Errors come back as a string ("" = fine).
#pragma once
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>
#include "tf_internal.h"
#include "tf_packed.h"
#include "tf_tiles_host.h"

namespace tfp {

// parity-blocked layout tables (tf_layout.hip.h), host mirror
struct HostLayout {
    int N = 0, NW = 0, RS = 0, MC = 1;
    int KS = 1 << 30, MP = 1;                                  // steps per part and parts of a cut walk (several ranks: shorter tasks)
    int cstart[4] = {}, csize[4] = {}, corder[4] = {}, wfirst[5] = {}, fullsec[4][4] = {}, gbase[4] = {};
    long long cbase[4] = {}, NP[4] = {}, NPtot = 0, RLS = 0;
    std::vector<int> cls, loc, sigma, ao, origI, clsI, cntA, kap0, kapF, rpoff, chunk_c0, chunk_width, chunk_cls, chunk_of, gk;
    std::vector<KInfo> kinfo;                                   // [4][N]
    std::vector<int> offE;                                      // [4][N]: offA + padded segment length
    int ke(int a, int xI) const { return cntA[(size_t)a * N + xI]; }
    int seclen(int c, int a, int iI) const { const int k = ke(a, iI); return k == 0 ? 0 : offE[(size_t)c * N + cstart[a] + k - 1]; }
    int row_shape(int c, int iI, int *secoff) const {           // section starts and the length of a class-c row with first index iI
        int tot = 0;
        for (int t = 0; t < 4; ++t) { const int a = corder[t]; secoff[a] = tot; tot += seclen(c, a, iI); }
        return tot;
    }
    bool task_exists(int c, int w, int iI) const { return kap0[(size_t)c * NW + w] < ke(chunk_cls[w] ^ c, iI); }
};

// Tables of the parity-blocked layout for the output AOs of a build (the NumPy model tests/layout_model.py builds the same tables).
// cls[k]: x/y parity class of output AO k (original order); parts: parts the walks of the Fock kernel are cut into (several ranks).
inline std::string build_layout(const std::vector<int> &cls, int parts, HostLayout &H)
{
    H = HostLayout();
    const int N = (int)cls.size(), PAD = TF_SEG_PAD;
    H.N = N; H.cls = cls;
    for (int k = 0; k < N; ++k) ++H.csize[cls[k]];
    int order[4] = {0, 1, 2, 3};
    std::stable_sort(order, order + 4, [&](int x, int y) { return H.csize[x] > H.csize[y]; });   // larger classes first (ties: class id)
    for (int t = 0, s0 = 0; t < 4; ++t) { H.corder[t] = order[t]; H.cstart[order[t]] = s0; s0 += H.csize[order[t]]; }
    H.loc.assign(N, 0); H.sigma.assign(N, 0); H.ao.assign(N, 0); H.origI.assign(N, 0); H.clsI.assign(N, 0);
    std::vector<int> cnt((size_t)4 * N, 0);                          // cnt[b][k]: class-b AOs with original index <= k
    {
        int seen[4] = {0, 0, 0, 0};
        for (int k = 0; k < N; ++k) {
            H.loc[k] = seen[cls[k]]++;
            H.sigma[k] = H.cstart[cls[k]] + H.loc[k];
            H.ao[k] = cls[k] | (H.loc[k] << 2);
            H.origI[H.sigma[k]] = k;
            H.clsI[H.sigma[k]] = cls[k];
            for (int b = 0; b < 4; ++b) cnt[(size_t)b * N + k] = seen[b];
        }
    }
    H.cntA.assign((size_t)4 * N, 0);
    for (int a = 0; a < 4; ++a)
        for (int x = 0; x < N; ++x) H.cntA[(size_t)a * N + x] = cnt[(size_t)a * N + H.origI[x]];
    H.kinfo.assign((size_t)4 * N, KInfo{0, 0});
    H.offE.assign((size_t)4 * N, 0);
    for (int c = 0; c < 4; ++c) {
        long long tot = 0;
        for (int t = 0; t < 4; ++t) {
            const int a = H.corder[t];
            H.fullsec[c][a] = (int)tot;
            long long off = 0;
            for (int kk = 0; kk < H.csize[a]; ++kk) {
                const int kI = H.cstart[a] + kk;
                const int n = cnt[(size_t)(a ^ c) * N + H.origI[kI]];
                H.kinfo[(size_t)c * N + kI] = KInfo{(int)off, n};
                off += (n + PAD - 1) / PAD * PAD;
                H.offE[(size_t)c * N + kI] = (int)off;
            }
            tot += off;
        }
        if (tot > 0x7fffffffLL / 8) return "basis too large for the packed layout's 32-bit row offsets";
        H.NP[c] = tot;
    }
    H.NPtot = 0; H.RLS = 0;
    for (int c = 0; c < 4; ++c) { H.cbase[c] = H.NPtot; H.NPtot += H.NP[c]; H.RLS = std::max(H.RLS, H.NP[c]); }
    // granule table: AO k of the segment that holds granule g of class c's pair index space
    {
        int gb = 0;
        for (int c = 0; c < 4; ++c) { H.gbase[c] = gb; gb += (int)(H.NP[c] / PAD); }
        H.gk.assign((size_t)std::max(gb, 1), 0);
        for (int c = 0; c < 4; ++c)
            for (int kI = 0; kI < N; ++kI) {
                const int a = H.clsI[kI];
                const int g0 = (H.fullsec[c][a] + H.kinfo[(size_t)c * N + kI].offA) / PAD, g1 = (H.fullsec[c][a] + H.offE[(size_t)c * N + kI]) / PAD;
                for (int g = g0; g < g1; ++g) H.gk[(size_t)H.gbase[c] + g] = kI;
            }
    }
    // column chunks: the internal columns cut at class boundaries and every TF_JKP_CW columns
    H.chunk_of.assign(N, 0);
    for (int b = 0; b < 4; ++b) {
        H.wfirst[b] = (int)H.chunk_cls.size();
        for (int lam0 = 0; lam0 < H.csize[b]; lam0 += TF_JKP_CW) {
            const int wd = std::min(TF_JKP_CW, H.csize[b] - lam0);
            for (int u = 0; u < wd; ++u) H.chunk_of[H.cstart[b] + lam0 + u] = (int)H.chunk_cls.size();
            H.chunk_cls.push_back(b); H.chunk_c0.push_back(H.cstart[b] + lam0); H.chunk_width.push_back(wd);
        }
    }
    H.wfirst[4] = (int)H.chunk_cls.size();
    H.NW = (int)H.chunk_cls.size();
    const int NW = H.NW;
    H.kap0.assign((size_t)4 * std::max(NW, 1), 0); H.kapF.assign((size_t)4 * std::max(NW, 1), 0); H.rpoff.assign((size_t)4 * std::max(NW, 1), 0);
    // row parts of a group / row: a dense [MC][N] block, MC = most chunks of one class; the task of chunk number s of its class writes
    // slot s at the internal index of k: rpoff[c][w] = s N + cstart[class of k] (+ kappa)
    H.MC = 1;
    for (int b = 0; b < 4; ++b) H.MC = std::max(H.MC, H.wfirst[b + 1] - H.wfirst[b]);
    H.RS = H.MC * N;
    {
        // Several ranks: a rank has 1/world of the tasks but every task walks as long as before, so the longest walks bound the pass
        // (N = 400, 8 ranks: 0.58 ms against 0.24 ms at perfect balance).  The walks are cut into MP parts of KS steps; the price is one
        // plane of column parts (and of Jd) per part.
        int longest = 1;
        for (int a = 0; a < 4; ++a) longest = std::max(longest, H.csize[a]);
        H.MP = std::max(1, std::min(parts, longest));
        H.KS = (longest + H.MP - 1) / H.MP;
    }
    for (int c = 0; c < 4; ++c) {
        for (int w = 0; w < NW; ++w) {
            const int b = H.chunk_cls[w], a = b ^ c, lam0 = H.chunk_c0[w] - H.cstart[b];
            const int cm = (c == 0) ? 1 : 0;
            int k0 = H.csize[a], kF = H.csize[a];
            for (int kk = H.csize[a] - 1; kk >= 0; --kk) {           // the counts are non-decreasing along a class
                const int n = H.kinfo[(size_t)c * N + H.cstart[a] + kk].cnt;
                if (n > lam0) k0 = kk;
                if (H.chunk_width[w] == TF_JKP_CW && n - cm >= lam0 + TF_JKP_CW) kF = kk;
            }
            H.kap0[(size_t)c * NW + w] = k0; H.kapF[(size_t)c * NW + w] = kF;
            H.rpoff[(size_t)c * NW + w] = (w - H.wfirst[b]) * N + H.cstart[a];
        }
    }
    return "";
}

// what the table builder of the tiles layout (tf_tiles_host.h) needs of the class ordering
inline tft::ClassInfo class_info(const HostLayout &H)
{
    tft::ClassInfo C;
    C.N = H.N;
    for (int q = 0; q < 4; ++q) { C.cstart[q] = H.cstart[q]; C.csize[q] = H.csize[q]; }
    C.clsI = H.clsI; C.origI = H.origI; C.cntA = H.cntA;
    return C;
}

// x/y parity class of every output AO (original order)
inline void ao_classes(const tf::Basis &bs, bool spherical, std::vector<int> &cls)
{
    cls.assign((size_t)(spherical ? bs.n_sph : bs.n_cart), 0);
    // every Cartesian component of a real spherical AO has the AO's x/y parity: the first one decides
    std::vector<double> blk;
    int o = 0;
    for (const auto &sh : bs.shells) {
        const int nout = spherical ? sh.nsph : sh.ncomp;
        if (spherical) tf::sph_block(sh.L, blk);
        for (int r = 0; r < nout; ++r) {
            int cc = r;
            if (spherical) {
                cc = 0;
                while (cc < sh.ncomp && blk[(size_t)r * sh.ncomp + cc] == 0.0) ++cc;
            }
            const int ca = sh.cart_off + cc;
            cls[o++] = (bs.ao_lmn[3 * ca] & 1) | ((bs.ao_lmn[3 * ca + 1] & 1) << 1);
        }
    }
}

// ---- row tables: the tensor rows a rank owns
struct RowTables {
    std::vector<TFInt2> row_ij;                 // original (i >= j) of every local row
    std::vector<int> rowmap;                    // [N (N + 1) / 2] -> local row or -1: keyed by (i, j) original; packed: by the unordered internal pair
    std::vector<long long> pair_first_row;      // [shell pairs]: first row of an owned pair in the order list_rows made (-1: not owned)
    std::vector<long long> rowoff;              // packed: start of the storage unit of row r in the tensor; [n_rows]: n_elems
    std::vector<int> rowsec;                    // packed: [n_rows + 1][6]: section starts; position in its storage unit, rows of the unit
    std::vector<int> rowlen;                    // packed: stored doubles of a row
    long long n_elems = 0;                      // packed: stored doubles
};
inline size_t ikey(int x, int y) { const int hi = std::max(x, y), lo = std::min(x, y); return (size_t)hi * (hi + 1) / 2 + lo; }

// the rows (i >= j) of the owned shell pairs, pair by pair; out_off / out_dim: output AOs of every shell
inline void list_rows(const std::vector<tf::Pair> &pairs, const std::vector<int> &out_off, const std::vector<int> &out_dim,
                      const std::vector<int> &my_pairs, int N, RowTables &R)
{
    R = RowTables();
    R.rowmap.assign((size_t)N * (N + 1) / 2, -1);
    R.pair_first_row.assign(pairs.size(), -1);
    std::vector<TFInt2> &row_ij = R.row_ij;
    for (int p : my_pairs) {
        const int A = pairs[p].A, B = pairs[p].B;
        R.pair_first_row[p] = (long long)row_ij.size();
        for (int x = 0; x < out_dim[A]; ++x)
            for (int y = 0; y < out_dim[B]; ++y) {
                const int i = out_off[A] + x, j = out_off[B] + y;
                if (i < j) continue;
                R.rowmap[(size_t)i * (i + 1) / 2 + j] = (int)row_ij.size();
                row_ij.push_back(TFInt2{i, j});
            }
    }
}

// packed layouts: the rows reordered for the layout H, their shapes and (unless the tensor is stored in tiles) their storage units
inline void pack_rows(const HostLayout &H, bool tiles, RowTables &R)
{
    const int N = H.N;
    std::vector<TFInt2> &row_ij = R.row_ij;
    std::vector<int> &rowmap = R.rowmap, &rowsec = R.rowsec, &rowlen = R.rowlen;
    std::vector<long long> &rowoff = R.rowoff;
    // owned rows in ascending internal (sigma(i), sigma(j)): rows that share i and the class of j are adjacent (the row groups of the
    // J/K kernel); rowmap is keyed by the unordered pair of internal indices
    {
        // (the keys sigma(i) N + sigma(j) are distinct: one pass over the N^2 key space instead of a comparison sort -- 3 ms at N = 400)
        std::vector<int> slot((size_t)N * N, -1);
        for (size_t r = 0; r < row_ij.size(); ++r) slot[(size_t)H.sigma[row_ij[r].x] * N + H.sigma[row_ij[r].y]] = (int)r;
        std::vector<TFInt2> sorted;
        sorted.reserve(row_ij.size());
        for (size_t k = 0; k < slot.size(); ++k)
            if (slot[k] >= 0) sorted.push_back(row_ij[(size_t)slot[k]]);
        row_ij.swap(sorted);
    }
    std::fill(rowmap.begin(), rowmap.end(), -1);
    rowoff.assign(row_ij.size() + 1, 0);
    rowsec.assign(6 * row_ij.size() + 6, 0);
    rowlen.assign(row_ij.size() + 1, 0);
    for (size_t r = 0; r < row_ij.size(); ++r) {
        const int i = row_ij[r].x, j = row_ij[r].y;
        rowmap[ikey(H.sigma[i], H.sigma[j])] = (int)r;
        if (!tiles) rowlen[r] = H.row_shape(H.cls[i] ^ H.cls[j], H.sigma[i], &rowsec[6 * r]);
    }
    if (tiles) return;
    // storage units: runs of up to 8 consecutive j of one class with the same i, cut from the top (the row groups of the kernel; its
    // groups of 4 for two densities are halves of them); the rows of a unit are interleaved segment by segment
    long long off = 0;
    for (long long r = (long long)row_ij.size() - 1; r >= 0;) {
        long long r0 = r;
        auto sI = [&](long long q) { return H.sigma[row_ij[q].x]; };
        auto sJ = [&](long long q) { return H.sigma[row_ij[q].y]; };
        while (r0 > 0 && sI(r0 - 1) == sI(r) && sJ(r0 - 1) == sJ(r0) - 1 && H.clsI[sJ(r0 - 1)] == H.clsI[sJ(r)] && r - r0 + 1 < TF_JKP_JBB) --r0;
        const int nr = (int)(r - r0 + 1);
        for (long long q = r0; q <= r; ++q) { rowoff[q] = off; rowsec[6 * q + 4] = (int)(q - r0); rowsec[6 * q + 5] = nr; }
        off += (long long)nr * rowlen[r0];
        r = r0 - 1;
    }
    rowoff[row_ij.size()] = off;
    R.n_elems = off;
}

// ---- work tables of the J/K kernel for groups of RB rows (8: one density per pass; 4: two)
struct JKWork {
    std::vector<JKGroup> groups;
    std::vector<int> gfirst;            // [2][N]: first / one-past-last group with i == a
    std::vector<JKSuper> supers;
    std::vector<JKTask> tasks;
    int bucket[4] = {0, 0, 0, 0};       // tasks [bucket[b], bucket[b + 1]) run with 4, 2, 1 waves per workgroup (b = 0, 1, 2)
    // the tasks a CLASS-DIAGONAL density needs (same order, same buckets): a row (i, j) of class c != 0 only meets P[j][l], P[j][k],
    // P[i][k], P[i][l] and the pair densities of class 0 -- every product of a task whose column class is neither i's nor j's is zero
    std::vector<JKTask> tasks_cd;
    int bucket_cd[4] = {0, 0, 0, 0};
    int nseg = 1;
    long long ypart_len = 0;
    JKJtPlan jp{};
};
// steps of a task: its stretch of the walk of its super-group along its chunk
inline int task_steps(const HostLayout &H, const JKSuper &sg, const JKTask &t)
{
    const int walk = H.ke(H.chunk_cls[t.w] ^ sg.c, sg.i) - H.kap0[(size_t)sg.c * H.NW + t.w];
    return std::min(H.KS, walk - t.part * H.KS);
}
// whether a class-diagonal density needs the task: its column class is i's or j's (or the rows are of class 0)
inline bool task_class_diagonal(const HostLayout &H, const JKSuper &sg, const JKTask &t)
{
    const int ci = H.clsI[sg.i], cj = ci ^ sg.c, cb = H.chunk_cls[t.w];
    return sg.c == 0 || cb == ci || cb == cj;
}
inline void build_jk_work(const HostLayout &H, const RowTables &rows, int RB, JKWork &T)
{
    T = JKWork();
    const int N = H.N;
    const std::vector<TFInt2> &row_ij = rows.row_ij;
    const std::vector<long long> &rowoff = rows.rowoff;
    const std::vector<int> &rowsec = rows.rowsec;
    std::vector<JKGroup> &groups = T.groups;
    std::vector<JKTask> &tasks = T.tasks;
    std::vector<JKSuper> &supers = T.supers;
    std::vector<int> &gfirst = T.gfirst;
    gfirst.assign(2 * (size_t)N, 0);
    long long ypart_len = 0;
    auto sI = [&](long long r) { return H.sigma[row_ij[r].x]; };
    auto sJ = [&](long long r) { return H.sigma[row_ij[r].y]; };
    // groups: runs of consecutive internal j of one class with the same i, largest j first
    for (long long r = (long long)row_ij.size() - 1; r >= 0;) {
        long long r0 = r;
        while (r0 > 0 && sI(r0 - 1) == sI(r) && sJ(r0 - 1) == sJ(r0) - 1 && H.clsI[sJ(r0 - 1)] == H.clsI[sJ(r)] && r - r0 + 1 < RB) --r0;
        JKGroup g{};
        g.i = sI(r); g.j0 = sJ(r0); g.nr = (int)(r - r0 + 1); g.r0 = (int)r0;
        g.c = H.clsI[g.i] ^ H.clsI[g.j0]; g.lamj0 = g.j0 - H.cstart[H.clsI[g.j0]];
        g.ub = rowoff[r0]; g.p0 = rowsec[6 * (size_t)r0 + 4]; g.unr = rowsec[6 * (size_t)r0 + 5];
        for (int a = 0; a < 4; ++a) g.secoff[a] = rowsec[6 * (size_t)r0 + a];
        groups.push_back(g);
        r = r0 - 1;
    }
    // (the reductions want the groups of one i contiguous: they are, the rows being sorted by i)
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const int a = groups[gi].i;
        if (gfirst[N + a] == gfirst[a]) gfirst[a] = (int)gi;
        gfirst[N + a] = (int)gi + 1;
    }
    // super-groups: up to TF_JKP_GPW * TF_JKP_W adjacent groups (TF_JKP_GPW per wave) with the same i and class share a workgroup and one Jt partial.  The kernel's
    // groups index into `groups`, so the super list may be reordered freely: by class, then by descending original i (the Jt
    // reduction needs those that reach an AO k to be a prefix of their class's list)
    for (size_t gi = 0; gi < groups.size();) {
        size_t ge = gi + 1;
        while (ge < groups.size() && groups[ge].i == groups[gi].i && groups[ge].c == groups[gi].c && ge - gi < TF_JKP_GPW * TF_JKP_W) ++ge;
        JKSuper sg{};
        sg.g0 = (int)gi; sg.ng = (int)(ge - gi); sg.c = groups[gi].c; sg.i = groups[gi].i;
        for (int a = 0; a < 4; ++a) sg.ke[a] = H.ke(a, sg.i);
        supers.push_back(sg);
        gi = ge;
    }
    std::stable_sort(supers.begin(), supers.end(), [&](const JKSuper &u, const JKSuper &v) {
        return u.c != v.c ? u.c < v.c : H.origI[u.i] > H.origI[v.i];
    });
    JKJtPlan jp{};
    for (size_t si = 0; si < supers.size(); ++si) {
        supers[si].yoff = ypart_len;
        ypart_len += H.NP[supers[si].c];
        ++jp.sfirst[supers[si].c + 1];
    }
    for (int c = 0; c < 4; ++c) {
        jp.sfirst[c + 1] += jp.sfirst[c];
        jp.bfirst[c + 1] = jp.bfirst[c] + (int)((H.NP[c] + TF_JKR_THREADS - 1) / TF_JKR_THREADS);
    }
    // tasks (super-group, chunk) that have at least one step, longest first: the hardware dispatches workgroups in this order
    std::vector<int> steps;
    for (size_t si = 0; si < supers.size(); ++si)
        for (int w = 0; w < H.NW; ++w)
            if (H.task_exists(supers[si].c, w, supers[si].i)) {
                const int walk = H.ke(H.chunk_cls[w] ^ supers[si].c, supers[si].i) - H.kap0[(size_t)supers[si].c * H.NW + w];
                for (int part = 0; part * H.KS < walk; ++part) {
                    tasks.push_back(JKTask{(int)si, w, part, 0});
                    steps.push_back(std::min(H.KS, walk - part * H.KS));
                }
            }
    {
        // workgroups of 4, 2 or 1 waves (two groups per wave): a rank of several holds few groups per (i, class), and a wave without
        // a group would only sit in the barriers of its workgroup and occupy a SIMD slot.  One launch per workgroup size; inside
        // a launch longest first.
        auto waves = [&](int t) {                                  // workgroup sizes TF_JKP_W, TF_JKP_W / 2, TF_JKP_W / 4 waves (at least one)
            const int nwv = (supers[tasks[t].super].ng + TF_JKP_GPW - 1) / TF_JKP_GPW;
            for (int b = 2; b >= 0; --b) if ((TF_JKP_W >> b) >= 1 && nwv <= (TF_JKP_W >> b)) return TF_JKP_W >> b;
            return TF_JKP_W;
        };
        std::vector<int> ord(tasks.size());
        std::iota(ord.begin(), ord.end(), 0);
        std::stable_sort(ord.begin(), ord.end(), [&](int u, int v) { return waves(u) != waves(v) ? waves(u) > waves(v) : steps[u] > steps[v]; });
        std::vector<JKTask> sorted(tasks.size());
        T.bucket[0] = 0; T.bucket[1] = T.bucket[2] = T.bucket[3] = (int)tasks.size();
        for (size_t t = 0; t < ord.size(); ++t) {
            sorted[t] = tasks[ord[t]];
            const int wv = waves(ord[t]);
            if (wv <= TF_JKP_W / 2 && T.bucket[1] == (int)tasks.size()) T.bucket[1] = (int)t;
            if (wv <= TF_JKP_W / 4 && T.bucket[2] == (int)tasks.size()) T.bucket[2] = (int)t;
        }
        if (T.bucket[2] < T.bucket[1]) T.bucket[1] = T.bucket[2];
        tasks.swap(sorted);
    }
    // the class-diagonal list: the same tasks in the same order without those whose column class is neither i's nor j's
    std::vector<JKTask> &tasks_cd = T.tasks_cd;
    tasks_cd.reserve(tasks.size());
    for (int b = 0; b < 4; ++b) T.bucket_cd[b] = 0;
    for (size_t t = 0; t < tasks.size(); ++t) {
        for (int b = 1; b < 4; ++b) if ((int)t == T.bucket[b]) T.bucket_cd[b] = (int)tasks_cd.size();
        if (task_class_diagonal(H, supers[tasks[t].super], tasks[t])) tasks_cd.push_back(tasks[t]);
    }
    for (int b = 1; b < 4; ++b) if (T.bucket[b] == (int)tasks.size()) T.bucket_cd[b] = (int)tasks_cd.size();
    T.nseg = std::max(1, std::min(TF_JKP_SEG, (int)supers.size() / 128));
    T.ypart_len = ypart_len;
    T.jp = jp;
}

// ---- the tables only the CONSUMERS of the tensor need besides the work tables
struct ConsumerTables {
    // rows listed class by class (the AO->MO transformation works on one class at a time: a row of class c is nonzero only in
    // the blocks (k of class a) x (l of class a ^ c)); position of a row in that order
    std::vector<int> class_rows, row_pos;
    long long class_row_off[5] = {0, 0, 0, 0, 0};      // rows of class c: class_rows[class_row_off[c] .. class_row_off[c + 1])
    // reduction table: the rows (z, x), z != x, listed by their second index x (internal): jrows[jptr[x] .. jptr[x + 1]) = (local
    // row, ORIGINAL first index of the row)
    std::vector<int> jptr;
    std::vector<TFInt2> jrows;
    std::vector<int> xorder;            // output rows of the exchange reduction, most partial vectors first
};
inline void build_class_rows(const HostLayout &H, const RowTables &rows, ConsumerTables &T)
{
    const std::vector<TFInt2> &row_ij = rows.row_ij;
    std::vector<int> &class_rows = T.class_rows, &row_pos = T.row_pos;
    class_rows.clear();
    row_pos.assign(row_ij.size(), 0);
    class_rows.reserve(row_ij.size());
    for (int c = 0; c < 4; ++c) {
        T.class_row_off[c] = (long long)class_rows.size();
        for (size_t r = 0; r < row_ij.size(); ++r)
            if ((H.cls[row_ij[r].x] ^ H.cls[row_ij[r].y]) == c) { row_pos[r] = (int)class_rows.size(); class_rows.push_back((int)r); }
    }
    T.class_row_off[4] = (long long)class_rows.size();
}
inline void build_reduction_lists(const HostLayout &H, const RowTables &rows, ConsumerTables &T)
{
    const int N = H.N;
    const std::vector<TFInt2> &row_ij = rows.row_ij;
    std::vector<int> &jptr = T.jptr, &xorder = T.xorder;
    std::vector<TFInt2> &jrows = T.jrows;
    jptr.assign((size_t)N + 1, 0);
    for (size_t r = 0; r < row_ij.size(); ++r) {
        const int iI = H.sigma[row_ij[r].x], jI = H.sigma[row_ij[r].y];
        if (iI != jI) ++jptr[jI + 1];
    }
    for (int x = 0; x < N; ++x) jptr[x + 1] += jptr[x];
    jrows.assign((size_t)std::max(1, jptr[N]), TFInt2{0, 0});
    {
        std::vector<int> fill(jptr.begin(), jptr.end() - 1);
        for (size_t r = 0; r < row_ij.size(); ++r) {            // (ascending local row: a fixed summation order)
            const int iI = H.sigma[row_ij[r].x], jI = H.sigma[row_ij[r].y];
            if (iI != jI) jrows[fill[jI]++] = TFInt2{(int)r, row_ij[r].x};
        }
    }
    // dispatch order of the exchange reduction: the output rows with the most partial vectors (rows listed under x + groups of x) first
    std::vector<long long> work((size_t)N, 0);
    for (int x = 0; x < N; ++x) work[x] = jptr[x + 1] - jptr[x];
    for (const TFInt2 &ij : row_ij) work[H.sigma[ij.x]] += 1;          // (8 rows of a group: weight 1/8 each would do; the order is what counts)
    xorder.assign((size_t)N, 0);
    std::iota(xorder.begin(), xorder.end(), 0);
    std::stable_sort(xorder.begin(), xorder.end(), [&](int a, int b) { return work[a] > work[b]; });
}

}  // namespace tfp
