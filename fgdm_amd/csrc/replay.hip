// Recorder and replay executor of recorded network walks (replay.h); the schedule itself is replay_plan.h's.
#include "replay.h"

#include <cstdio>
#include <cstring>

// ---- recorder: the list the launch sites of this thread record into
static thread_local RecWalk* g_rec = nullptr;

RecWalk* fgdm_record_into(RecWalk* walk) {
    RecWalk* before = g_rec;
    g_rec = walk;
    return before;
}
bool fgdm_recording() { return g_rec != nullptr; }

void fgdm_record(std::function<int(hipStream_t)> run) {
    g_rec->emplace_back();
    g_rec->back().run = std::move(run);
}
void fgdm_record(std::function<int(hipStream_t)> run, const void* key, FgdmGroupFn group, const void* args, size_t nbytes,
                 unsigned grid_x, unsigned long long shape) {
    fgdm_record(std::move(run));
    if (!group || !args || nbytes > FGDM_GROUP_BLOB) return;      // no grouped form: the launch replays alone
    RecOp& o = g_rec->back();
    o.key = key; o.group = group; o.grid_x = grid_x; o.shape = shape;
    memcpy(o.args, args, nbytes);
}
void fgdm_record_bracket_begin(int cls, double w, double bytes, const char* tag) {
    g_rec->emplace_back();
    RecOp& o = g_rec->back();
    o.kind = RecOp::PROF_BEGIN; o.cls = cls; o.w = w; o.bytes = bytes;
    snprintf(o.tag, sizeof(o.tag), "%s", tag);
}
void fgdm_record_bracket_end() {
    g_rec->emplace_back();
    g_rec->back().kind = RecOp::PROF_END;
}

// ---- units: one op, or a profiler bracket around exactly one launch; `launch` = the op the planner matches on
namespace {
struct Unit { size_t first, last, launch; };

void units_of(const RecWalk& v, std::vector<Unit>& units, PlanWalk& plan) {
    for (size_t i = 0; i < v.size();) {
        const bool bracket = v[i].kind == RecOp::PROF_BEGIN && i + 2 < v.size() && v[i + 1].kind == RecOp::RUN && v[i + 2].kind == RecOp::PROF_END;
        const Unit u{i, bracket ? i + 2 : i, bracket ? i + 1 : i};
        const RecOp& o = v[u.launch];
        units.push_back(u);
        plan.push_back(o.kind == RecOp::RUN && o.group ? PlanUnit{(uint64_t)(uintptr_t)o.key, o.grid_x, o.shape} : PlanUnit{0, 0, 0});
        i = u.last + 1;
    }
}
}  // namespace

// ---- executor
int fgdm_replay(const std::vector<RecWalk*>& walks, int chunk, hipStream_t s, LaunchTimer& timer, ReplayStats& stats) {
    std::vector<std::vector<Unit>> units(walks.size());
    std::vector<PlanWalk> plan(walks.size());
    for (size_t w = 0; w < walks.size(); ++w) units_of(*walks[w], units[w], plan[w]);
    std::vector<int32_t> steps;
    replay_plan_chunked(plan.data(), (int)plan.size(), chunk, FGDM_MAX_GROUP, REPLAY_LOOK, steps);
    for (size_t i = 0; i < steps.size(); i += 1 + 2 * (size_t)steps[i]) {
        const int n = steps[i];
        const int32_t* m = &steps[i + 1];      // (walk, unit) x n
        if (n == 1) {
            RecWalk& v = *walks[m[0]];
            const Unit& u = units[m[0]][m[1]];
            for (size_t k = u.first; k <= u.last; ++k) {
                RecOp& o = v[k];
                if (o.kind == RecOp::PROF_BEGIN) timer.begin(o.cls, s, o.w, o.tag, o.bytes);
                else if (o.kind == RecOp::PROF_END) timer.end(s);
                else { ++stats.replayed; const int rc = o.run(s); if (rc != FGDM_OK) return rc; }
            }
            continue;
        }
        // fused: one bracket (all the problems' work), one launch
        const void* av[FGDM_MAX_GROUP];
        double w = 0.0, bytes = 0.0;
        const RecOp* br = nullptr;
        for (int k = 0; k < n; ++k) {
            const RecWalk& v = *walks[m[2 * k]];
            const Unit& u = units[m[2 * k]][m[2 * k + 1]];
            av[k] = v[u.launch].args;
            if (u.first != u.last) { w += v[u.first].w; bytes += v[u.first].bytes; if (!br) br = &v[u.first]; }
        }
        const RecOp& lead = (*walks[m[0]])[units[m[0]][m[1]].launch];
        if (br) timer.begin(br->cls, s, w, br->tag, bytes);
        const int rc = lead.group(av, n, lead.grid_x, s);
        if (rc != FGDM_OK) return rc;
        if (br) timer.end(s);
        ++stats.fused; ++stats.replayed; stats.problems += n;
    }
    return FGDM_OK;
}
