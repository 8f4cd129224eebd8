// Anchor ("seed") stage of the per-read correction on the device: the work of getSeeds
// (reference: src/Graph.cpp:3-482) after the exact k-mer scan -- masking (:102-191), 1-edit k-mer search
// (:193, Bifrost searchSequence inexact [A2]), solid/weak split (:201-219), overlap filter (:221-239),
// keep_non_overlap (src/Alignment.cpp:1017-1199) and the adjacent-run consistency check (:329-372).
// One wavefront owns one long read (mask, finalize) or one tile of 64 window positions (inexact probes).
#ifndef RTK_SEEDS_H
#define RTK_SEEDS_H

// one header per program, in the order of the stage
#include "rtk_seed_types.h"
#include "rtk_colour_sets.h"
#include "rtk_seed_mask.h"
#include "rtk_seed_window.h"
#include "rtk_seed_enum.h"
#include "rtk_seed_seeded.h"
#include "rtk_seed_finalize.h"

#endif
