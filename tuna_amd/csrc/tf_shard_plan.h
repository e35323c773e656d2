// tf_shard_plan.h -- which rank owns which bra shell pair of a sharded tensor (include/tunafock.h: tf_shard_plan, tf_shard_plan_pairs).
// Deterministic, so every rank computes the same plan without communication.  Plain C++17, no HIP: tests/ctx_model compiles it with
// g++ (tests/test_ctx_plan.py pins the owners).  DESIGN.md section 3.2.
#pragma once
#include <algorithm>
#include <numeric>
#include <vector>

#include "tf_packed.h"             // packed_row_len: the weight proxy of the packed layout

// Longest-processing-time assignment of row blocks (bra shell pairs) to ranks: heaviest block first, always to
// the least loaded rank.
inline void shard_plan(const std::vector<long long> &weight, int world, std::vector<int> &owner)
{
    const int n = (int)weight.size();
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return weight[x] > weight[y]; });
    std::vector<long long> load(world, 0);
    owner.assign(n, 0);
    for (int p : order) {
        const int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        load[r] += weight[p];
        owner[p] = r;
    }
}

// The plan of tf_build_eri.  `forced`: the value of TF_SHARD_PLAN (null: not set), read by the caller.
inline void shard_plan_pairs(const std::vector<int> &dim, bool packed, int world, const char *forced, std::vector<int> &owner)
{
    const int ns = (int)dim.size();
    std::vector<long long> off(ns + 1, 0);
    for (int s = 0; s < ns; ++s) off[s + 1] = off[s] + dim[s];
    owner.assign((size_t)ns * (ns + 1) / 2, 0);
    std::vector<long long> load(world, 0);
    std::vector<long long> w;
    // WHOLE bra shells per rank when that balances (round 3): a rank then holds complete runs of j for its rows i -- super-groups as full
    // as on one GPU, and an eighth of the super-groups, so that the Jt partials and their reduction shrink with the shard.  (With every A
    // cut into `world` segments each rank keeps a short run of j under EVERY i: at N = 400 on 8 ranks the per-rank reduction stayed at
    // 0.08 ms -- as many super-groups per rank as on one GPU -- and the J/K kernel ran on one-group workgroups.)  Longest-processing-time
    // over the shells' weights; taken if the heaviest rank is within 3 % of the mean, else the segment plan below.  TF_SHARD_PLAN=segments
    // / shells forces one of the two (identically on every rank, of course).
    {
        const bool force_seg = forced && forced[0] == 's' && forced[1] == 'e', force_sh = forced && forced[0] == 's' && forced[1] == 'h';
        if (world > 1 && !force_seg) {
            std::vector<long long> wA(ns, 0);
            long long total = 0;
            for (int A = 0; A < ns; ++A) {
                for (long long i = off[A]; i < off[A + 1]; ++i)
                    for (long long j = 0; j <= i; ++j) wA[A] += packed ? packed_row_len(i, j) : 1;
                total += wA[A];
            }
            std::vector<int> ord(ns);
            std::iota(ord.begin(), ord.end(), 0);
            std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return wA[x] > wA[y]; });
            std::vector<long long> ld(world, 0);
            std::vector<int> rankA(ns, 0);
            for (int A : ord) {
                const int r = (int)(std::min_element(ld.begin(), ld.end()) - ld.begin());
                ld[r] += wA[A];
                rankA[A] = r;
            }
            const long long heaviest = *std::max_element(ld.begin(), ld.end());
            if (force_sh || (double)heaviest * world <= 1.03 * (double)total) {
                for (int A = 0; A < ns; ++A)
                    for (int B = 0; B <= A; ++B) owner[(size_t)A * (A + 1) / 2 + B] = rankA[A];
                return;
            }
        }
    }
    for (int A = ns - 1; A >= 0; --A) {                           // heaviest rows first
        w.assign(A + 1, 0);
        long long total = 0;
        for (int B = 0; B <= A; ++B) {
            long long wb = 0;
            for (long long i = off[A]; i < off[A + 1]; ++i)
                for (long long j = off[B]; j < off[B + 1] && j <= i; ++j) wb += packed ? packed_row_len(i, j) : 1;
            w[B] = wb; total += wb;
        }
        // `world` contiguous segments of B with (nearly) equal weight
        struct Seg { int b0, b1; long long wt; };
        std::vector<Seg> segs;
        int b = 0;
        long long cum = 0;
        for (int sgi = 1; sgi <= world; ++sgi) {
            const long long target = (long long)((__int128)total * sgi / world);
            Seg sg{b, b, 0};
            while (b <= A && (sgi == world || cum + w[b] / 2 <= target)) { cum += w[b]; sg.wt += w[b]; ++b; }
            sg.b1 = b;
            segs.push_back(sg);
        }
        std::stable_sort(segs.begin(), segs.end(), [](const Seg &x, const Seg &y) { return x.wt > y.wt; });
        std::vector<int> ranks(world);
        std::iota(ranks.begin(), ranks.end(), 0);
        std::stable_sort(ranks.begin(), ranks.end(), [&](int x, int y) { return load[x] < load[y]; });
        for (int k = 0; k < world; ++k) {
            const Seg &sg = segs[k];
            for (int B = sg.b0; B < sg.b1; ++B) owner[(size_t)A * (A + 1) / 2 + B] = ranks[k];
            load[ranks[k]] += sg.wt;
        }
    }
}
