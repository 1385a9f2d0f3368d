// Every environment variable the native library reads: one table (name, default, meaning) and one parser.
//
// A knob's value is the variable's text, or the default's where the variable is not set, through atoi (knob_int, knob_on) or
// atof: text that is no number reads as 0, and an on/off knob is off for exactly the texts atoi reads as 0 (the empty one
// included).  A default of nullptr marks a knob that carries text, not a number (knob_text: nullptr while it is not set).
//
// WHEN a knob is read is part of its meaning:
//   knob_once   the launcher knobs: once per process, all of them at the first use of any one (never before the first launch)
//   knob_int /  at every call: the knobs of fgdm_create (two engines of one process may differ in them), FGDM_PAIR_DEBUG
//   knob_text   (fgdm_destroy), FGDM_PROF_DUMP (fgdm_profile_end), FGDM_BENCH_DATA_SCALE (the fgdm_bench_* entries)
// README.md lists the same names (tests/test_lib_abi.py holds the two tables to each other).
#pragma once
#include "common.h"
#include <array>
#include <cstdlib>

#define FGDM_STR_(x) #x
#define FGDM_STR(x) FGDM_STR_(x)

//  id, variable, default, meaning
#define FGDM_KNOBS(X)                                                                                                          \
    X(ATTN_PP, "FGDM_ATTN_PP", "1", "0: the four-wave attention kernel where the eight-wave ping-pong one would run")           \
    X(ATTN_DQ, "FGDM_ATTN_DQ", "3", "long self-attention, d = 40: 3 = two-strand kernel, 32-wide V^T P^T; 1 = 16-wide; 0 = off") \
    X(ATTN_DQ80, "FGDM_ATTN_DQ80", "1", "0: the ping-pong kernel instead of the two-strand one at d = 64 / 80")                 \
    X(ATTN_ABL, "FGDM_ATTN_ABL", "0", "ablation instantiations of the two-strand kernel (tools/bench_attention.py only)")       \
    X(ATTN_CROSS, "FGDM_ATTN_CROSS", "4", "query chunks per wave of the text-token kernel (65 - 96 keys); 0 = off")             \
    X(ATTN_CROSS_LONG, "FGDM_ATTN_CROSS_LONG", "8", "query chunks per wave of the key-resident kernel (97 - 256 keys); 0 = off") \
    X(IGEMM_EPI_PATHS, "FGDM_IGEMM_EPI_PATHS", "1", "0: the general GEMM epilogue instead of the host-selected straight-line paths") \
    X(IGEMM_HALO, "FGDM_IGEMM_HALO", "1", "0: per-tap K loop instead of the halo-tile loop (stride-1 3x3 convolutions, split K too)") \
    X(IGEMM_MFMA32, "FGDM_IGEMM_MFMA32", "0", "1: automatic tile choices take the 32x32x16 MFMA instantiations")                \
    X(IGEMM_OTHER_WIDTHS, "FGDM_IGEMM_OTHER_WIDTHS", "1", "0: widths 128 / 256 / 512 back on the 2-stage kernel")               \
    X(IGEMM_PERSIST, "FGDM_IGEMM_PERSIST", "1", "GEGLU projections: 1 = persistent, tiles round-robin; 2 = contiguous runs; 0 = off") \
    X(IGEMM_PIPE, "FGDM_IGEMM_PIPE", "1", "0: the phase-locked K loop instead of the software-pipelined one")                   \
    X(IGEMM_UP_PHASE, "FGDM_IGEMM_UP_PHASE", "1", "0: Upsample convs as the 3x3 walk over the virtual upsampled image, not four 2x2 phase GEMMs") \
    X(IGEMM_SMALL_M, "FGDM_IGEMM_SMALL_M", "1", "0: linears with a thin 128-row grid stay on 128 x 320 tiles")                  \
    X(IGEMM_SMALL_TILES, "FGDM_IGEMM_SMALL_TILES", "1", "0: the 8x8 level's linears back on the 2-stage kernel")                \
    X(IGEMM_STATS64, "FGDM_IGEMM_STATS64", "1", "0: the 64 x 160 tile leaves the LayerNorm partial sums to the row-statistics pass") \
    X(SPLITK_FAT, "FGDM_SPLITK_FAT", "1", "0: split K four ways on 128 x 320 tiles at the 8x8 level only")                      \
    X(PAIR_FAT_TILES, "FGDM_PAIR_FAT_TILES", "1", "0: grouped launches keep the tile a single problem would take")              \
    X(GN_REG, "FGDM_GN_REG", "1024", "largest pixel count per sample of the register-resident GroupNorm; 0 = off")              \
    X(GN_REG_NG, "FGDM_GN_REG_NG", "4", "widest slice of the register-resident GroupNorm, in groups")                           \
    X(GN_FUSED_MAXKB, "FGDM_GN_FUSED_MAXKB", "64", "largest LDS slice (KB) of the single-kernel GroupNorm; 0 = always two kernels") \
    X(GN_CHUNK, "FGDM_GN_CHUNK", FGDM_STR(GN_PIX_PER_CHUNK), "pixels per partial-sum chunk of the two-kernel GroupNorm (multiples of 64)") \
    X(LN_FOLD, "FGDM_LN_FOLD", "1", "fgdm_create; 0: the transformer blocks' LayerNorms as kernels of their own")               \
    X(TWIN_STREAMS, "FGDM_TWIN_STREAMS", "0", "fgdm_create; 1: the ControlNets on a second stream next to the UNet encoder")    \
    X(PAIR_LAUNCH, "FGDM_PAIR_LAUNCH", "1", "fgdm_create; 0: no grouped launches of twin layers")                               \
    X(GROUP_MAX, "FGDM_GROUP_MAX", FGDM_STR(FGDM_MAX_GROUP), "fgdm_create; problems per grouped launch, clamped to [2, FGDM_MAX_GROUP]") \
    X(GN_GROUP, "FGDM_GN_GROUP", "1", "fgdm_create; 0: single-pass GroupNorm launches stay out of the grouped launches")        \
    X(PAIR_DEBUG, "FGDM_PAIR_DEBUG", nullptr, "set (to anything): fgdm_destroy prints how many replayed launches were fused")   \
    X(PROF_DUMP, "FGDM_PROF_DUMP", nullptr, "path: fgdm_profile_end writes the per-shape time table there")                     \
    X(BENCH_DATA_SCALE, "FGDM_BENCH_DATA_SCALE", "1", "atof; scale of the random operands of fgdm_bench_igemm / _attention")

enum Knob {
#define X(id, name, dflt, meaning) KNOB_##id,
    FGDM_KNOBS(X)
#undef X
    KNOB_COUNT
};
struct KnobDef { const char* name; const char* dflt; const char* meaning; };
inline constexpr KnobDef KNOB_TABLE[KNOB_COUNT] = {
#define X(id, name, dflt, meaning) {name, dflt, meaning},
    FGDM_KNOBS(X)
#undef X
};

inline const char* knob_text(Knob k) {
    const char* v = getenv(KNOB_TABLE[k].name);
    return v ? v : KNOB_TABLE[k].dflt;
}
inline int knob_int(Knob k) { return atoi(knob_text(k)); }
inline bool knob_on(Knob k) { return knob_int(k) != 0; }
inline int knob_once(Knob k) {
    static const std::array<int, KNOB_COUNT> v = [] {
        std::array<int, KNOB_COUNT> a{};
        for (int i = 0; i < KNOB_COUNT; ++i)
            if (KNOB_TABLE[i].dflt) a[i] = knob_int((Knob)i);
        return a;
    }();
    return v[k];
}
