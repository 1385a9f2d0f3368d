// Stand-alone host program around fgdm_amd/csrc/replay_plan.h for a sanitizer run of the planner (no HIP, no Python):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/replay_plan_check.cpp -o replay_plan_check && ./replay_plan_check
// It replays the cases of tests/test_replay_plan.py, checks every schedule's invariants and the expected number of grouped launches.
#include "../fgdm_amd/csrc/replay_plan.h"

#include <cstdio>
#include <set>
#include <utility>

static const PlanUnit A{7, 40, 0}, B{8, 40, 0}, C{9, 16, 3}, D{11, 2, 0}, PLAIN{0, 0, 0};
static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the schedule's invariants; returns the number of grouped launches
static int check(const std::vector<PlanWalk>& walks, int group_max = 5, int chunk = 0) {
    std::vector<int32_t> out;
    replay_plan_chunked(walks.data(), (int)walks.size(), chunk, group_max, REPLAY_LOOK, out);
    std::vector<long> last(walks.size(), -1);
    size_t units = 0, total = 0;
    int groups = 0;
    for (const PlanWalk& w : walks) total += w.size();
    for (size_t i = 0; i < out.size(); i += 1 + 2 * (size_t)out[i]) {
        const int n = out[i];
        EXPECT(n >= 1 && n <= group_max && i + 1 + 2 * (size_t)n <= out.size());
        std::set<int> members;
        for (int k = 0; k < n; ++k, ++units) {
            const int w = out[i + 1 + 2 * k], u = out[i + 2 + 2 * k];
            EXPECT(w >= 0 && w < (int)walks.size() && u == last[w] + 1 && u < (int)walks[w].size());      // in order, none twice
            last[w] = u;
            members.insert(w);
            const PlanUnit &x = walks[w][u], &l = walks[out[i + 1]][out[i + 2]];
            if (n > 1) EXPECT(x.key != 0 && x.key == l.key && x.grid_x == l.grid_x && x.shape == l.shape);
        }
        EXPECT((int)members.size() == n);
        groups += n > 1;
    }
    EXPECT(units == total);
    for (size_t w = 0; w < walks.size(); ++w) EXPECT(last[w] + 1 == (long)walks[w].size());
    return groups;
}

int main() {
    const PlanWalk six{A, B, C, A, D, B};
    EXPECT(check({six, six}) == 6);
    EXPECT(check({PlanWalk(3, PlanUnit{7, 40, 0}), PlanWalk(3, PlanUnit{7, 41, 0})}) == 0);
    EXPECT(check({PlanWalk(3, PlanUnit{7, 40, 5}), PlanWalk(3, PlanUnit{7, 40, 6})}) == 0);
    EXPECT(check({PlanWalk(3, PlanUnit{0, 40, 0}), PlanWalk(3, PlanUnit{0, 40, 0})}) == 0);
    for (const PlanUnit& other : {PLAIN, B}) {
        PlanWalk near(REPLAY_LOOK - 1, other), far(REPLAY_LOOK, other);
        near.push_back(A); far.push_back(A);
        EXPECT(check({{A}, near}) == 1);
        EXPECT(check({{A}, far}) == 0);
    }
    EXPECT(check({{A, B}, {PLAIN, PLAIN, PLAIN, A, B}}) == 2);
    EXPECT(check({{A}, {A, B, PLAIN, C}, {A, B, C, PLAIN}}) == 3);
    EXPECT(check(std::vector<PlanWalk>(7, PlanWalk{A, PLAIN, B})) == 2);
    const PlanWalk w{A, B, PLAIN, C};
    EXPECT(check(std::vector<PlanWalk>(4, w), 5, 2) == 6);
    EXPECT(check(std::vector<PlanWalk>(3, w), 5, 2) == 3);
    EXPECT(check(std::vector<PlanWalk>(4, w), 5, 0) == 3);
    EXPECT(check(std::vector<PlanWalk>(4, w), 2, 0) == 3);      // two surplus walks whole, then pairs
    EXPECT(check({}) == 0);
    EXPECT(check({{}, {}}) == 0);
    EXPECT(check({{A, PLAIN, A}}) == 0);
    EXPECT(check({{}, {A, B}, {}, {A, B}}) == 2);
    EXPECT(check({six, six}, 1) == 0);
    printf(failures ? "replay_plan_check: %d FAILED\n" : "replay_plan_check: all cases passed\n", failures);
    return failures ? 1 : 0;
}
