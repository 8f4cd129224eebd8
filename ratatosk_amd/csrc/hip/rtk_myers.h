// Bit-parallel Myers/Hyyro edit distance on one wavefront, with the observable behaviour of the reference's
// vendored edlib (reference: src/edlib.cpp:141-296 edlibAlign; :547-704 semi-global; :730-931 NW; :945-1144
// traceback; :1164-1216 traceback/Hirschberg switch; :1234-1399 Hirschberg; src/Common.hpp:262-276 equalities).
//
// Layout: one 64-bit word of the query per lane; the carry between vertically adjacent words travels lane->lane+1
// with one __shfl_up per step, so the wave sweeps the DP matrix along anti-diagonals ("step s: lane l works on
// column s-l"). Queries longer than 64 words are processed in row blocks of 64 words; the horizontal deltas leaving
// a block are parked in a per-column int8 array and picked up by lane 0 of the next block.
//
// Band (edlib.cpp:194-212 k doubling, :778-915 firstBlock/lastBlock): the big NW problems -- bounded distances and the half passes of
// the Hirschberg recursion, i.e. the whole-read alignment of phasing() -- only compute the Ukkonen band of their k, at word granularity;
// what lies outside is an upper bound, so distances, split rows and tracebacks are those of the unbanded matrix (why: DESIGN_HISTORY.md 3.9).
// Where edlib doubles k, an unknown-distance problem runs with a guess and once more with the score it found if that exceeds the guess. Two schedules:
//   * ring (band <= 4000 diagonals, one wave): lane = word & 63; a word enters the band at the bottom, leaves it at the top 64 + band
//     columns later and its lane takes word + 64; a pass is n + W steps whatever the number of row blocks (rtk_myers_ring);
//   * blocks (wider bands): the 4096-row blocks of rtk_myers_block each sweep the columns [4096 b + dlo, 4096 b + 4095 + dhi] only.
// Small problems (one row block) and the stored sweeps of the tracebacks compute whole columns: the wave sweeps them in n + W steps anyway.
// The query profile is indexed by character class (15 IUPAC letters); any other byte is compared on the fly.
//
// This header is the list of the aligner's parts in reading order; each has its own guard and includes what it needs. The order is also the order in which
// the compiler meets the out-of-line device functions, which is the order of the code object: rtk_myers_distance stands in front of rtk_myers_walk for that reason.
// One RTK_SIM conditional per header at most (the device schedules and the simulator's stand-ins for them are whole files), plus the one that picks
// the device's rtk_myers_walk or the simulator's.
#ifndef RTK_MYERS_H
#define RTK_MYERS_H
#include "rtk_acgt.h"           // alphabet: character classes, which are equal, 2-bit packing
#include "rtk_myers_types.h"    // modes, MyersScratch and who uses which buffer as what, the traceback table, results, the in-memory bound, the work-area carve
#include "rtk_myers_step.h"     // Advance_Block in 64 and 32 bits, the query profile
#include "rtk_myers_band.h"     // geometry of the Ukkonen band (host and device)
#include "rtk_myers_sim.h"      // RTK_SIM only: the simulator's column-by-column passes, sweeps and walk
#include "rtk_myers_sweep.h"    // device: the branch-free sweeps over one row block
#include "rtk_myers_blocks.h"   // device: a pass as work items -- row blocks, the ring
#include "rtk_myers_coop.h"     // RTK_MULTIWAVE: the items of a pass or round on the waves of a workgroup
#include "rtk_myers_pass.h"     // device: the generic pass and the banded pass, which pick the schedule
#include "rtk_myers_distance.h" // edlib's distance entry, SHW by column, the SHW / HW end rule, the last column of a pass
#include "rtk_myers_walk.h"     // the walk over a stored table, the last move alone, sweep + walk
#include "rtk_myers_lvl.h"      // device: Hirschberg level by level, the half passes of a level side by side in the lanes
#include "rtk_myers_align.h"    // obtainAlignment on an explicit stack, edlib's path entry, the saved-sweep pair
#endif
