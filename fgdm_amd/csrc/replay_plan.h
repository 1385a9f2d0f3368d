// The schedule of a lockstep replay of recorded walks (replay.h), as a pure function: plain host C++, no HIP, no engine state.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// a partner's member of a group is looked for among the next REPLAY_LOOK units it has not run yet
constexpr int REPLAY_LOOK = 24;

// What the planner knows of a unit (one recorded op, or a profiler bracket around exactly one launch): two units may share a
// grouped launch when their key (non-zero: the kernel's grouped form), grid and shape are equal.  key 0: not fusable.
struct PlanUnit { uint64_t key; uint32_t grid_x; uint64_t shape; };
typedef std::vector<PlanUnit> PlanWalk;

// Appends the schedule of walks [w0, w1) to `out`, a step being  n, (walk, unit) x n:  n == 1 runs that unit alone, n >= 2 launches
// the units' grouped form once (the leader first).  Every walk keeps its own order (the nets are independent of each other):
//  * walks beyond `group_max` replay whole and ungrouped, the last walk first, before anything else;
//  * the first walk leads: its fusable unit is grouped with the first unit of equal key, grid and shape that each later walk
//    holds within `look` units of where it stands; what such a partner holds in front of its member runs first, in its own order;
//  * when the leader runs out, the next walk leads.
inline void replay_plan(const PlanWalk* walks, int w0, int w1, int group_max, int look, std::vector<int32_t>& out) {
    auto alone = [&](int w, size_t u) { out.insert(out.end(), {1, (int32_t)w, (int32_t)u}); };
    for (; w1 - w0 > group_max && w1 > w0; --w1)
        for (size_t u = 0; u < walks[w1 - 1].size(); ++u) alone(w1 - 1, u);
    std::vector<size_t> at(w1 > w0 ? w1 - w0 : 0, 0);       // the next unit of walk w0 + i
    std::vector<int32_t> grp;
    for (int lead = w0; lead < w1; ++lead) {
        const PlanWalk& A = walks[lead];
        for (size_t& a = at[lead - w0]; a < A.size();) {
            grp.assign({(int32_t)lead, (int32_t)a});
            for (int m = lead + 1; m < w1 && A[a].key; ++m) {
                const PlanWalk& B = walks[m];
                for (size_t j = at[m - w0]; j < B.size() && j < at[m - w0] + (size_t)look; ++j)
                    if (B[j].key == A[a].key && B[j].grid_x == A[a].grid_x && B[j].shape == A[a].shape) {
                        grp.insert(grp.end(), {(int32_t)m, (int32_t)j});
                        break;
                    }
            }
            if (grp.size() < 4) { alone(lead, a++); continue; }
            for (size_t k = 2; k < grp.size(); k += 2)
                for (size_t& b = at[grp[k] - w0]; b < (size_t)grp[k + 1]; ++b) alone(grp[k], b);
            out.push_back((int32_t)(grp.size() / 2));
            out.insert(out.end(), grp.begin(), grp.end());
            for (size_t k = 0; k < grp.size(); k += 2) at[grp[k] - w0] = (size_t)grp[k + 1] + 1;
        }
    }
}

// `n_walks` walks cut into runs of at most `chunk` for replay_plan, as apply_model does when FGDM_GROUP_MAX is below the number of
// walks: run r holds the walks [r * chunk, min(n_walks, (r + 1) * chunk)); chunk <= 0: one run
inline void replay_plan_chunked(const PlanWalk* walks, int n_walks, int chunk, int group_max, int look, std::vector<int32_t>& out) {
    if (chunk <= 0) chunk = n_walks > 0 ? n_walks : 1;
    for (int w0 = 0; w0 < n_walks; w0 += chunk) replay_plan(walks, w0, w0 + chunk < n_walks ? w0 + chunk : n_walks, group_max, look, out);
}
