// Recorded network walks and their lockstep replay (the launch sites' side is in common.h: "deferred launches").
// While a list is selected (fgdm_record_into), every launch, copy and profiler bracket edge of the walk becomes a RecOp in it
// instead of being enqueued; fgdm_replay then runs several such walks side by side on one stream, in the order replay_plan.h
// decides, launches of equal key, grid and shape fused into the grouped form of their kernel.
#pragma once
#include "common.h"
#include "replay_plan.h"

#include <vector>

struct RecOp {
    RecOp() {}                           // (user-provided: `args` is not cleared for every op built; it is read only behind `group`)
    enum Kind { RUN, PROF_BEGIN, PROF_END } kind = RUN;
    std::function<int(hipStream_t)> run;
    const void* key = nullptr;           // RUN of a launch that has a grouped form: what fgdm_record was given
    FgdmGroupFn group = nullptr;
    unsigned grid_x = 0;
    unsigned long long shape = 0;
    alignas(8) char args[FGDM_GROUP_BLOB];
    int cls = 0;                         // PROF_BEGIN
    double w = 0, bytes = 0;
    char tag[56] = {0};
};
typedef std::vector<RecOp> RecWalk;

// Selects the list that records from now on (nullptr: launches are enqueued again); returns the one selected before.
RecWalk* fgdm_record_into(RecWalk* walk);
// The edges of a profiler bracket around the next launch, as ops of the walk being recorded
void fgdm_record_bracket_begin(int cls, double w, double bytes, const char* tag);
void fgdm_record_bracket_end();

// The kernel timer a replay drives (engine.hip: Prof)
struct LaunchTimer {
    virtual void begin(int cls, hipStream_t s, double w, const char* tag, double nbytes) = 0;
    virtual void end(hipStream_t s) = 0;
protected:
    ~LaunchTimer() = default;
};
struct ReplayStats { long replayed = 0, fused = 0, problems = 0; };      // all replayed launches; fused launches; problems in those

// Replays `walks` on `s` in runs of `chunk` walks (replay_plan_chunked), every walk in its own order.  A fused step takes ONE
// bracket: the members' work and bytes summed, class and tag of the first member that has a bracket.
int fgdm_replay(const std::vector<RecWalk*>& walks, int chunk, hipStream_t s, LaunchTimer& timer, ReplayStats& stats);
