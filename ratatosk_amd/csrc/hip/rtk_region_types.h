// Region stage, types: the region descriptors and batch views, the wave's work area (RegionScratch) with the names of its buffers, the
// overflow codes, lap slots, alignment sites and the size-class table, and the layout of the work area in its slab. No reference routine
// is restated here; the buffers stand for the locals of correctSequence and its `correct` lambda (reference: src/Correction.cpp:159-958),
// Path (src/Path.hpp) and ResultCorrection (src/ResultCorrection.hpp).
#ifndef RTK_REGION_TYPES_H
#define RTK_REGION_TYPES_H

#include "rtk_myers.h"
#include "rtk_seeds.h"
#include "rtk_types.h"
#include "rtk_wave.h"

// ------------------------------------------------------------------------------------------------ data
struct RegionDesc { // one entry per output segment of a read, in read order
    uint32_t read;
    uint32_t kind;     // RTK_RG_*
    uint32_t i_solid;  // index of the left solid anchor (interior / tail), unused otherwise
    uint32_t prev_pos; // where the previous segment stopped in the read
    uint64_t seg_off;  // out: offset of the segment in the segment pool (sequence bytes, then quality bytes)
    uint32_t seq_len, qual_len; // out
    uint32_t status;   // out: non-zero = scratch overflow, redo with a bigger arena
    uint32_t pad;
};
#define RTK_RG_WHOLE_MAX 0   // read returned unchanged, qualities all 'I' (every window solid)
#define RTK_RG_WHOLE_MIN 1   // read returned unchanged, qualities all '!' (no solid anchor / too short)
#define RTK_RG_HEAD 2        // before the first solid anchor (reverse-complement correction, src/Correction.cpp:776-797)
#define RTK_RG_GAP 3         // between two consecutive solid anchors that are not adjacent (:803-935)
#define RTK_RG_TAIL 4        // after the last solid anchor, corrected forward (:940-950)
#define RTK_RG_TAIL_COPY 5   // read ends on a solid anchor (:951-955)

struct RegionBatch {
    U<RegionDesc*> regions; U<uint64_t> regions_cap; U<unsigned long long*> n_regions;
    U<uint64_t*> r_first; U<uint32_t*> r_count;   // per read: its slice of `regions`
    U<char*> seq_rc;                           // reverse complement of every read (same offsets as seq)
    U<char*> qual_rev;                         // pass 2: every read's quality string reversed (q_bw of src/Correction.cpp:186,198)
    U<char*> seg_pool; U<uint64_t> seg_cap; U<unsigned long long*> seg_top;
    U<unsigned long long*> next_region;        // dequeue head of the persistent region kernel
    U<uint32_t*> eorder;                       // the regions that need no graph walk (k_regions_easy), in any order; their number is n_heavy[2]
    U<uint32_t*> rorder; U<unsigned long long*> n_heavy; // dequeue order of the region kernel: the heavy regions (long gaps, read heads / tails) from the front, the light ones from the back (k_region_order); [0] heavy, [1] light
    U<unsigned long long*> n_overflow;         // regions that ran out of scratch in the last launch
    U<uint32_t*> horder; // the regions the lane kernel handed on to the wave kernel; their number is n_heavy[4]
    U<uint32_t*> lorder; U<unsigned long long*> next_lane; U<uint32_t> lane_max_gap; // the regions of the lane-per-region kernel (k_regions_lanes): gaps under lane_max_gap bases, by size class; their number is n_heavy[3]; 0: no such class
    U<char*> out_pool; U<uint64_t> out_cap; U<unsigned long long*> out_top;
    U<uint64_t*> out_off; U<uint32_t*> out_seq_len; U<uint32_t*> out_qual_len; // per read
    U<uint64_t*> st_off;                       // per segment: quality bytes << 32 | characters of its read in front of it (k_stitch)
};

// ------------------------------------------------------------------------------------------------ names of the work buffers
// Every buffer of RegionScratch is addressed by a name. A buffer with two roles in turn has one name per role, with the same value; the
// table says who owns it when. "correct" is one rtk_correct_region call: side lists -> colours -> path search -> assembly -> fixAmbiguity
// -> trim. A gap region runs: correct (forward) -> rtk_strand2_skippable -> [rtk_park_walk -> correct (second strand) -> reverse complement
// -> consensus] -> emit; a head region: correct (second strand) -> reverse complement -> emit; a tail region: correct (forward) -> emit.
//
// buffer        name                      written by                         read by                           live
// rbuf[0], [1]  RTK_RB_FW_SEQ, _QUAL      correct (forward)                  driver, strand-2 rule, consensus  forward correct .. emit
// rbuf[2], [3]  RTK_RB_BW_SEQ, _QUAL      correct (second strand), rev.compl. driver, consensus                second correct .. emit
// rbuf[4], [5]  RTK_RB_OUT_SEQ, _QUAL     driver (rtk_app)                   rtk_emit_segment                  whole region
// rbuf[6]       RTK_RB_RC_TMP             rtk_rc_reverse_complement          the same call                     inside that call
//               RTK_RB_CONS_SEQ           consensus; driver (raw fallback)   driver (audit, emit_minus_k)      consensus .. emit
// rbuf[7]       RTK_RB_PARK_MOVES         rtk_park_walk                      consensus (`resume`)              park walk .. consensus's resume
//               RTK_RB_CONS_QUAL          consensus; driver (raw fallback)   driver (audit, emit_minus_k)      consensus .. emit
// str[0]        RTK_STR_CAND              path search; correct's assembly; driver (same-unitig shortcut)       one candidate / path string at a time
//               RTK_STR_AMB_QUERY         rtk_fix_ambiguity                  the same call                     inside that call
// str[1]        RTK_STR_PATH              DFS, BFS pop (path being scored)   rtk_score_path, _qual             one scoring at a time
//               RTK_STR_AMB_SUB           rtk_fix_ambiguity                  the same call                     inside that call
// str[2]        RTK_STR_QUAL              rtk_score_path_qual                DFS / BFS (Path::setQuality)      one scoring at a time
// str[3]        RTK_STR_SWEEP_STASH       rtk_myers_nw_and_save (DFS)        rtk_myers_path_from_saved         one DFS call
//               RTK_STR_CONS_MOVES_FW     consensus                          consensus (CigCur)                inside the consensus
// str[4]        RTK_STR_CONS_MOVES_BW     consensus                          consensus (CigCur)                inside the consensus
//               RTK_STR_PROBE             latency probe of a -DRTK_PROF build, in front of the region program  inside the probe
// bm[0], [1]    RTK_BM_FW, RTK_BM_BW      correct (corrected old positions)  strand-2 rule, consensus          as rbuf[0..3]
// bm[2]         RTK_BM_RC_TMP             rtk_rc_reverse_complement          the same call                     inside that call
// list[0..2]    RTK_L_SIDE_LEFT, _RIGHT, _MIDDLE  correct (side lists: u32 unitigs, flag bytes in the upper half)  colours   side lists .. end of colours
// list[0], [1]  RTK_L_BFS_PATHS, _NEW     rtk_explore_paths (v, v_tmp)       the same call                     one BFS call
// list[2], [3]  RTK_L_DFS_T, RTK_L_DFS_NT rtk_explore_subgraph               rtk_explore, rtk_explore_paths    one DFS call .. the next
// list[4]       RTK_L_DFS_STACK           rtk_explore_subgraph               the same call                     one DFS call
// list[3..5]    RTK_L_COL_VALS, _KEYS, _SLOT_OF  colour programs (candidate anchors: quota, key, slot)   the same     inside colours
// list[5]       RTK_L_PARTIAL             rtk_extract_semi_weak (dead ends)  correct (select_best)             path search .. assembly
// list[6..10]   RTK_L_AMB ..              rtk_amb_collect, rtk_fix_ambiguity (rtk_ambiguity.h lists the five)  assembly .. fixAmbiguity
// set[0]        RTK_SET_ALL_PIDS          colours (forward correct only)     path search of BOTH strands       colours .. end of the region
// set[3]        RTK_SET_ALL_PIDS_ALT      general colour program: all_pids alternates between the two while it grows, and ends in set[0]
// set[1], [2]   RTK_SET_UNION_A, _B       general colour program: ping-pong of a class's union; the bit-vector programs' second sort buffer,
//               RTK_SET_CS_SORT, RTK_SET_CS_TAGS, RTK_SET_CB_IDS, RTK_SET_CB_STORE   gathered ids, tags and vector store (rtk_colours.h)
// set[4]        RTK_SET_PICKED            rtk_first_shared (the ids one anchor adds)                            inside colours
// set[7], [8]   RTK_SET_CUR_A, _B         general colour program: curr_pid, ping-pong                           inside colours
// set[9]        RTK_SET_UNION_TMP         rtk_set_union (b \ a)              the same call                     inside that call
// wp[0]         RTK_WP_REGION             rtk_extract_semi_weak (the running path)                              path search
// wp[1]         RTK_WP_BFS                rtk_explore_paths; RTK_WP_REPEATS_PATH: rtk_fix_repeats (P), at the end of that call
// wp[2]         RTK_WP_DFS                rtk_explore_subgraph, the pending pop of rtk_explore_paths; RTK_WP_REPEATS_TRIAL: rtk_fix_repeats (E)
// wp[3]         RTK_WP_REPEATS_CYCLE      rtk_fix_repeats (R: the unitig list of one turn; its ums only)
// arena[0..2]   RTK_ARENA_REGION, _BFS, _DFS  path records of one correct / one rtk_explore_paths call / one rtk_explore_subgraph call; every
//                                         level is reset (top = 0) where its call begins
// arena[2]      RTK_ARENA_COL_SETS          general colour program: its set expressions, as slices            inside colours (the DFS level is free there)
// arena[0]      RTK_ARENA_COL_AUDIT         rtk_choose_colors (RTK_CM_AUDIT): the first answer's list          inside colours (the path search resets it after)
// loc.len[..]   RTK_LEN_*                 lengths of rbuf[4..7] and of the string / quality that correct is assembling (words rtk_app updates)
// loc.best[..]  RTK_BEST_ID, _END         rtk_select_best's answer in correct
// loc.an[..]    RTK_AN_*                  the read's solid / weak anchors, forward and reverse-complemented   whole region
// loc.rc[..]    RTK_RES_FW, RTK_RES_BW    the two ResCorr (pointers into rbuf[0..3], bm[0..1])                 whole region
// loc.side[..]  RTK_SIDE_*                the three SideList (pointers into list[0..2])                       side lists .. end of colours
// The read program of pass 2 (rtk_phasing.h; k_phase, k_phase_long) runs in the same work area with no region in progress: RTK_RB_PHASE_*,
// RTK_BM_PHASE_*, RTK_L_PHASE_*, RTK_ARENA_PHASE_FILTERS.
//
// Hand-overs, as invariants:
//  H1 rbuf[6]: rtk_rc_reverse_complement has returned before the consensus is called; nothing else uses the buffer.
//  H2 rbuf[7]: only rtk_park_walk writes RTK_RB_PARK_MOVES, and only from the forward trim (RTK_PARK_EAGER: inside it) to the decision about the second strand. The consensus copies
//     the parked moves to str[3] / str[4] (`resume`) before its first append to RTK_RB_CONS_QUAL; the exits that append earlier (`take`)
//     return without reading moves. A region that skips its second strand never walks the park (TrimPark::pending stays set).
//  H3 str[0], str[1]: fixAmbiguity runs after correct has appended the last path string, and the trim after fixAmbiguity.
//  H4 list[3]: the colour programs end before the path search begins (s.top[RTK_ARENA_REGION] = 0 in rtk_correct_region marks the border);
//     list[0..2] pass from the side lists to the path search at the same point.
//  H5 set[0]: written by the colour selection of the region's first correct call (rc == nullptr); a gap region's second call (rc != nullptr) reads it, so nothing
//     between the two calls may write set[0]. The temporaries of the colour programs are all other members of `set`.
//  H6 arena levels 2 and 0 under the colour selection: see RTK_ARENA_COL_SETS, RTK_ARENA_COL_AUDIT above.
enum RtkRbuf { RTK_RB_FW_SEQ = 0, RTK_RB_FW_QUAL = 1, RTK_RB_BW_SEQ = 2, RTK_RB_BW_QUAL = 3, RTK_RB_OUT_SEQ = 4, RTK_RB_OUT_QUAL = 5,
               RTK_RB_RC_TMP = 6, RTK_RB_CONS_SEQ = 6, RTK_RB_PARK_MOVES = 7, RTK_RB_CONS_QUAL = 7, RTK_RB_N = 8,
               RTK_RB_PHASE_SEQ = 0, RTK_RB_PHASE_QUAL = 1 };
enum RtkStr { RTK_STR_CAND = 0, RTK_STR_AMB_QUERY = 0, RTK_STR_PATH = 1, RTK_STR_AMB_SUB = 1, RTK_STR_QUAL = 2, RTK_STR_SWEEP_STASH = 3,
              RTK_STR_CONS_MOVES_FW = 3, RTK_STR_CONS_MOVES_BW = 4, RTK_STR_PROBE = 4, RTK_STR_N = 5 };
enum RtkBm { RTK_BM_FW = 0, RTK_BM_BW = 1, RTK_BM_RC_TMP = 2, RTK_BM_N = 3,
             RTK_BM_PHASE_RM = 0, RTK_BM_PHASE_NEW = 1, RTK_BM_PHASE_COV = 2 };
enum RtkList { RTK_L_SIDE_LEFT = 0, RTK_L_SIDE_RIGHT = 1, RTK_L_SIDE_MIDDLE = 2,
               RTK_L_BFS_PATHS = 0, RTK_L_BFS_NEW = 1, RTK_L_DFS_T = 2, RTK_L_DFS_NT = 3, RTK_L_DFS_STACK = 4, RTK_L_PARTIAL = 5,
               RTK_L_COL_VALS = 3, RTK_L_COL_KEYS = 4, RTK_L_COL_SLOT_OF = 5,
               RTK_L_AMB = 6, RTK_L_AMB_SAFE = 7, RTK_L_AMB_ALL = 8, RTK_L_AMB_UNITIG = 9, RTK_L_AMB_LINKED = 10, RTK_L_N = 11,
               RTK_L_PHASE_RUN_POS = 0, RTK_L_PHASE_RUN_UNITIG = 1, RTK_L_PHASE_NBITS = 2, RTK_L_PHASE_STATE = 3 };
enum RtkSet { RTK_SET_ALL_PIDS = 0, RTK_SET_UNION_A = 1, RTK_SET_UNION_B = 2, RTK_SET_ALL_PIDS_ALT = 3, RTK_SET_PICKED = 4,
              RTK_SET_CUR_A = 7, RTK_SET_CUR_B = 8, RTK_SET_UNION_TMP = 9, RTK_SET_N = 10, // (5 and 6 are free)
              // (the ping-pongs are `x ^ 3`: RTK_SET_UNION_A ^ 3 == RTK_SET_UNION_B, RTK_SET_ALL_PIDS ^ 3 == RTK_SET_ALL_PIDS_ALT)
              RTK_SET_CS_SORT = 1, RTK_SET_CS_TAGS = 2, RTK_SET_CB_IDS = 1, RTK_SET_CB_STORE = 2 };
enum RtkWp { RTK_WP_REGION = 0, RTK_WP_BFS = 1, RTK_WP_DFS = 2, RTK_WP_REPEATS_PATH = 1, RTK_WP_REPEATS_TRIAL = 2, RTK_WP_REPEATS_CYCLE = 3, RTK_WP_N = 4 };
enum RtkArena { RTK_ARENA_REGION = 0, RTK_ARENA_BFS = 1, RTK_ARENA_DFS = 2, RTK_ARENA_N = 3,
                RTK_ARENA_COL_AUDIT = 0, RTK_ARENA_COL_SETS = 2, RTK_ARENA_PHASE_FILTERS = 0 };
enum RtkLocLen { RTK_LEN_OUT_SEQ = 0, RTK_LEN_OUT_QUAL = 1, RTK_LEN_CONS_SEQ = 2, RTK_LEN_CONS_QUAL = 3, RTK_LEN_CORR_SEQ = 4, RTK_LEN_CORR_QUAL = 5, RTK_LEN_N = 6 };
enum RtkLocBest { RTK_BEST_ID = 0, RTK_BEST_END = 1, RTK_BEST_N = 2 };
enum RtkLocAnchors { RTK_AN_SOLID = 0, RTK_AN_WEAK = 1, RTK_AN_SOLID_RC = 2, RTK_AN_WEAK_RC = 3, RTK_AN_N = 4 };
enum RtkLocRes { RTK_RES_FW = 0, RTK_RES_BW = 1, RTK_RES_N = 2 };
enum RtkLocSide { RTK_SIDE_LEFT = 0, RTK_SIDE_RIGHT = 1, RTK_SIDE_MIDDLE = 2, RTK_SIDE_N = 3 };

// ------------------------------------------------------------------------------------------------ overflow codes
// What a region ran out of: RegionScratch::ovf_word, handed to the host as RegionDesc::status (non-zero: the region is redone with bigger
// work areas; the trace prints a histogram by number). 1 and 2 are written by the alignment code, which only knows its MyersScratch.
enum RtkOvf {
    RTK_OVF_NONE = 0,
    RTK_OVF_ALIGN_CAP = 1,     // rtk_myers.h, rtk_myers_lvl.h: a capacity of MyersScratch
    RTK_OVF_ALIGN_OPTIMUM = 2, // rtk_myers.h: inconsistent optimum in a traceback (cannot happen for a correct distance)
    RTK_OVF_ARENA = 3,         // arena_cap: a level of the path arenas
    RTK_OVF_PATH_LOAD = 4,     // a path record larger than a working path (um_cap, str_cap)
    RTK_OVF_PATH_UNITIGS = 5,  // um_cap: unitigs of a working path
    RTK_OVF_PATH_QUAL = 6,     // str_cap: quality string of a working path
    RTK_OVF_STRING = 7,        // str_cap: a string buffer (the read program: or bm_words)
    RTK_OVF_LIST = 8,          // list_cap
    RTK_OVF_SET = 9,           // set_cap
    RTK_OVF_BITMAP = 10,       // bm_words
    RTK_OVF_AMB = 11,          // rtk_ambiguity.h: list_cap / str_cap under the SNP annotations
    RTK_OVF_CONS_STALL = 11,   // the consensus makes no progress (would loop forever in the reference as well)
    RTK_OVF_SEG_POOL = 12,     // seg_cap: the segment pool of the batch
    RTK_OVF_REPEAT_QUAL = 14   // rtk_fix_repeats: a path without qualities (std::string::replace would throw in the reference)
};

// ------------------------------------------------------------------------------------------------ lap slots (-DRTK_PROF)
// RTK_PL(s, slot) books every cycle since the previous lap on `slot`. The numbers are those of the profiles/ files:
//  0 DRIVER_DISPATCH   1 DRIVER_SAME_UNITIG  2 REGION_PROLOGUE   3 REGION_SIDE_LISTS     4 REGION_COLOURS   5 SEMIWEAK_GLUE
//  6 PATHS_PROLOGUE    7 EXPLORE_PREFIX      8 DFS_POP           9 DFS_COLOUR_OK        10 DFS_T_EXTEND    11 DFS_T_STRING
// 12 DFS_T_SWEEP      13 DFS_T_COMMIT       14 DFS_NT_EXTEND    15 DFS_NT_REST          16 DFS_POST_SCORE  17 DFS_POST_STRING
// 18 DFS_POST_QUAL    19 DFS_POST_COMMIT    20 PATHS_AFTER_EXPLORE  21 PATHS_SELECT     22 SEMIWEAK_MERGE  23 REGION_RESTART
// 24 REGION_ASSEMBLE  25 REGION_FIX_AMBIGUITY  26 REGION_TRIM   27 DRIVER_STRAND2       28 CONS_ENTRY      29 CONS_FW_PATH
// 30 CONS_BW_PATH     31 CONS_MERGE         32 CONS_FINAL       33 DRIVER_EMIT_PREP     34 DEQUEUE         35 EMIT
// 36 .. 39 free       40 PROBE_COLD         41 PROBE_WARM       42 PROBE_SLAB           43 PROBE_SAMPLES   44 .. 47 free
// (40 .. 43: the in-situ latency probes of k_regions, rtk_pipeline_run.inc; 43 counts samples, not cycles.) The host's legend is `pn` in
// region_trace_report.
enum RtkLap {
    RTK_LAP_DRIVER_DISPATCH = 0, RTK_LAP_DRIVER_SAME_UNITIG = 1, RTK_LAP_REGION_PROLOGUE = 2, RTK_LAP_REGION_SIDE_LISTS = 3, RTK_LAP_REGION_COLOURS = 4,
    RTK_LAP_SEMIWEAK_GLUE = 5, RTK_LAP_PATHS_PROLOGUE = 6, RTK_LAP_EXPLORE_PREFIX = 7, RTK_LAP_DFS_POP = 8, RTK_LAP_DFS_COLOUR_OK = 9,
    RTK_LAP_DFS_T_EXTEND = 10, RTK_LAP_DFS_T_STRING = 11, RTK_LAP_DFS_T_SWEEP = 12, RTK_LAP_DFS_T_COMMIT = 13, RTK_LAP_DFS_NT_EXTEND = 14,
    RTK_LAP_DFS_NT_REST = 15, RTK_LAP_DFS_POST_SCORE = 16, RTK_LAP_DFS_POST_STRING = 17, RTK_LAP_DFS_POST_QUAL = 18, RTK_LAP_DFS_POST_COMMIT = 19,
    RTK_LAP_PATHS_AFTER_EXPLORE = 20, RTK_LAP_PATHS_SELECT = 21, RTK_LAP_SEMIWEAK_MERGE = 22, RTK_LAP_REGION_RESTART = 23, RTK_LAP_REGION_ASSEMBLE = 24,
    RTK_LAP_REGION_FIX_AMBIGUITY = 25, RTK_LAP_REGION_TRIM = 26, RTK_LAP_DRIVER_STRAND2 = 27, RTK_LAP_CONS_ENTRY = 28, RTK_LAP_CONS_FW_PATH = 29,
    RTK_LAP_CONS_BW_PATH = 30, RTK_LAP_CONS_MERGE = 31, RTK_LAP_CONS_FINAL = 32, RTK_LAP_DRIVER_EMIT_PREP = 33, RTK_LAP_DEQUEUE = 34, RTK_LAP_EMIT = 35,
    RTK_LAP_PROBE_COLD = 40, RTK_LAP_PROBE_WARM = 41, RTK_LAP_PROBE_SLAB = 42, RTK_LAP_PROBE_SAMPLES = 43,
    RTK_LAP_N = 48
};
static_assert(RTK_LAP_N == RTK_CNT_PROF_END - RTK_CNT_PROF, "lap slots: the counter map holds one word per slot");

// ------------------------------------------------------------------------------------------------ alignment sites (simulator census)
// RTK_SITE(site) names the call site of the alignments that follow (rtk_sim_census.h); profiles/r06_alignment_sites.txt and DESIGN.md §3.2
// cite the numbers. Rows 20 .. 31 of the census table are not call sites: the simulator keeps other counts there (DFS nodes, colour sizes).
enum RtkSite {
    RTK_SITE_NONE = 0,
    RTK_SITE_SCORE_TERMINAL = 1,      // rtk_score_path: terminal path, NW
    RTK_SITE_SCORE_REF_IN_PATH = 2,   // rtk_score_path: non-terminal path at least as long as the read window, HW of the window in the path
    RTK_SITE_SCORE_PATH_IN_REF = 3,   // rtk_score_path: shorter non-terminal path, HW of the path in the window
    RTK_SITE_PATH_QUAL = 4,           // rtk_score_path_qual: SHW path
    RTK_SITE_EXPLORE_PREFIX = 5,      // rtk_explore: where the path so far ends in the window, SHW
    RTK_SITE_SELECT_NT = 6,           // rtk_explore: several non-terminal sub-paths
    RTK_SITE_RESIZE_BEST = 7,         // rtk_resize_to_best
    RTK_SITE_REPEATS_PATH = 8,        // rtk_fix_repeats: the path as it came
    RTK_SITE_REPEATS_TURN = 9,        // rtk_fix_repeats: one more turn through a cycle
    RTK_SITE_SELECT_BFS = 10,         // rtk_explore_paths: several results
    RTK_SITE_SELECT_PARTIAL_RETRY = 11, // rtk_correct_region: best partial path, search goes on from a weak anchor
    RTK_SITE_SELECT_PARTIAL = 12,     // rtk_correct_region: best partial path, final
    RTK_SITE_TRIM_FALLBACK = 13,      // rtk_correct_region: the trim as a distance call
    RTK_SITE_CONS_FW = 14, RTK_SITE_CONS_BW = 15, RTK_SITE_CONS_FINAL = 16, // rtk_generate_consensus
    RTK_SITE_FIX_AMBIGUITY = 17,      // rtk_fix_ambiguity
    RTK_SITE_TRIM_STORED = 18, RTK_SITE_TRIM_COLUMN = 19 // rtk_trim_by_column: with / without the stored sweep
};

// ------------------------------------------------------------------------------------------------ size-class table
// RegionScratch::hist, region time by size class (trace): four blocks of eight classes, class b = rtk_gap_class(gap length) for a gap
// region, RTK_GAP_CLASS_HEAD_TAIL for a head / tail region.
// Slot 31 has two users: it is the running count of DFS calls of the wave (rtk_explore_subgraph adds 1; k_regions takes differences of it)
// AND bin RTK_H_DFS + RTK_GAP_CLASS_HEAD_TAIL, the DFS calls of head / tail regions (k_regions adds the difference). The printed figure
// of that bin is therefore wrong; left as it is here (a change of the trace's behaviour).
enum RtkHist { RTK_H_CYCLES = 0, RTK_H_REGIONS = 8, RTK_H_STRAND2 = 16, RTK_H_DFS = 24, RTK_H_DFS_RUNNING = 31, RTK_H_N = 32 };
enum { RTK_GAP_CLASS_HEAD_TAIL = 7, RTK_GAP_CLASSES = 8 };
static_assert(RTK_H_N == RTK_CNT_HIST_END - RTK_CNT_HIST, "size-class table: the counter map holds one word per slot");
// (a macro: as a function, inlined, the compiler arranges the table update of rtk_region_program differently. Give it a plain local.)
#define rtk_gap_class(gap_len) ((gap_len) < 40 ? 0 : (gap_len) < 64 ? 1 : (gap_len) < 128 ? 2 : (gap_len) < 256 ? 3 : (gap_len) < 512 ? 4 : (gap_len) < 1024 ? 5 : 6)

struct RegionScratchCfg { ScratchCfg my; uint32_t set_cap, um_cap, str_cap, list_cap, memo_cap, bm_words; uint64_t arena_cap; };

struct WPath { U<UMap*> ums; U<char*> qual; U<uint32_t> n, l, qlen; }; // mutable working path

// anchors of a read in one orientation, side lists of chooseColors, result of one `correct` call (functions: rtk_region_paths.h, rtk_colours.h, rtk_region_result.h)
struct Anchors { U<const uint32_t*> pos; U<const uint64_t*> hit; U<const uint64_t*> hits_by_pos; U<uint32_t> n, L; U<int> rev; U<int> k; };
struct SideList { uint32_t* u; uint8_t* nb; uint32_t n, cap; };
struct ResCorr { char* seq; char* qual; uint32_t seq_len, qual_len; uint64_t* bm; uint32_t old_len; bool is_corrected; uint32_t n_all; int all_set; };
// Locals of the region drivers that travel by reference (rtk_correct_region, rtk_generate_consensus, rtk_choose_colors): kept in the
// header (LDS in the kernels) instead of the wave's stack, where every wave-uniform word is a 256-byte row per store and per load
// state of one rtk_correct_region call that its three parts hand on (side lists + colours | path search | assembly + trim)
struct RegionCall { const char* s_read; const char* q_read; uint64_t complete; UMap um1, um2; uint32_t s_len, p1, p2, first_pos, len_weak_region, lw_lo, lw_hi, n_all, n_partial, n_amb, has_end_pt, found_first, lrc; };
// the forward trim of a gap region, kept for the consensus (rtk_trim_by_column): the alignment NW(rbuf[RTK_RB_FW_SEQ][0, len), raw region of n characters), distance dist, whose
// path ends in last_move. pending: nobody has walked the path yet, and rtk_park_walk makes it when a consensus is going to run -- from the stored sweep (RTK_PARK_TABLE,
// table generation gen), or, where the trim kept only the last column of its sweep (RTK_PARK_NO_TABLE), from a second, stored sweep of the same pair; else
// nm moves are parked in rbuf[RTK_RB_PARK_MOVES] (nm = 0 and not pending: nothing parked)
struct TrimPark { uint32_t nm, len; int32_t dist; uint32_t n, last_move, pending, gen; };
enum { RTK_PARK_TABLE = 1u, RTK_PARK_NO_TABLE = 2u };
struct DriverLocals { Anchors an[RTK_AN_N]; ResCorr rc[RTK_RES_N]; SideList side[RTK_SIDE_N]; uint32_t len[RTK_LEN_N]; int best[RTK_BEST_N]; MyersSaved saved; RegionCall call; TrimPark park; MyersResult trim; };

struct RegionScratch {
    MyersScratch my;
    // (who owns which member of the arrays when: the table above)
    U<uint32_t*> set[RTK_SET_N]; U<uint32_t> set_cap;
    U<char*> arena[RTK_ARENA_N]; U<uint64_t> arena_cap; U<uint64_t> top[RTK_ARENA_N];
    WPath wp[RTK_WP_N]; U<uint32_t> um_cap;
    U<char*> str[RTK_STR_N]; U<uint32_t> str_cap;
    U<char*> rbuf[RTK_RB_N];
    U<uint64_t*> list[RTK_L_N]; U<uint32_t> list_cap;
    U<uint32_t*> memo_u; U<uint8_t*> memo_v; U<uint32_t> memo_cap; U<uint32_t> memo_n;
    U<uint64_t*> bm[RTK_BM_N]; U<uint32_t> bm_words;
    UL<uint32_t*> overflow; U<uint32_t> ovf_word; // the flag itself, next to the header (same memory: LDS in the kernels)
    DriverLocals loc;
    U<unsigned long long> cnt[RTK_RC_N]; // event counts, then cycles: RtkRegionCnt (rtk_types.h)
    U<unsigned long long> fine[RTK_FINE_N]; // developer cycle counters printed with RTK_TRACE: RtkRegionFine (rtk_types.h)
#ifdef RTK_PROF
    U<unsigned long long> prof[RTK_LAP_N]; U<unsigned long long> prof_t; // developer build (-DRTK_PROF): lap profile of the region program, every cycle of a wave attributed to one slot (RTK_PL, RtkLap)
#endif
#ifndef RTK_SLIM_HDR
    U<unsigned long long> hist[RTK_H_N]; // region time by size class (RtkHist): [RTK_H_CYCLES + b] cycles, [RTK_H_REGIONS + b] regions, [RTK_H_STRAND2 + b] regions that needed the reverse strand too, [RTK_H_DFS + b] DFS calls
#endif
};
#ifdef RTK_SLIM_HDR // A/B build: header of 1 KB (20 waves per CU fit next to a 7 KB set buffer); the size-class table is not kept
#define RTK_HIST_ADD(sc, i, v) ((void)0)
#define RTK_HIST_GET(sc, i) 0ull
#else
#define RTK_HIST_ADD(sc, i, v) ((sc).hist[i] += (v))
#define RTK_HIST_GET(sc, i) ((sc).hist[i])
#endif
#ifdef RTK_PROF
#define RTK_PL(sc, i) do { const unsigned long long t_ = rtk_clock(); (sc).prof[i] += t_ - (sc).prof_t; (sc).prof_t = t_; } while (0)
#else
#define RTK_PL(sc, i) ((void)0)
#endif

// The views of a launch, ONE copy in device memory per batch (written by k_set_ctx in front of the kernels that read it). The wave
// programs read them through RCtx: a per-wave copy on the wave's stack costs 64 lanes x the struct in scratch memory (the stack is
// interleaved per lane), 45 KB per wave that every `c.g.x` then fetches a 256-byte row of.
struct LaunchCtx { GraphView g; OptsView o; BatchView bv; RegionBatch rb; };

struct RCtx { // everything a region program needs
    const GraphView& g; const OptsView& o; const BatchView& bv; const RegionBatch& rb; // -> the LaunchCtx of the launch
    UL<RegionScratch*> sc;
    U<int> k;
};

// the header of the wave's work area: in LDS in every kernel that runs the region / read programs (k_regions, k_phase, k_phase_long)
RTK_DEV RegionScratch& rtk_hdr(const RCtx& c) { RegionScratch* p = c.sc; RTK_ASSUME_LDS(p); return *p; }

// ------------------------------------------------------------------------------------------------ scratch layout
RTK_HD uint64_t region_scratch_bytes(const RegionScratchCfg& c) {
    uint64_t b = scratch_bytes(c.my);
    b += 4ull * RTK_SET_N * c.set_cap + 1ull * RTK_ARENA_N * c.arena_cap + 1ull * RTK_WP_N * (sizeof(UMap) * c.um_cap + c.str_cap) + (1ull * RTK_STR_N + RTK_RB_N) * c.str_cap;
    b += 8ull * RTK_L_N * c.list_cap + 5ull * c.memo_cap + 8ull * RTK_BM_N * c.bm_words + sizeof(RegionScratch) + 1024;
    return (b + 255) / 256 * 256;
}

// The RegionScratch header (pointers into the slab + the mutable control words: arena tops, working-path lengths, overflow flag,
// counters) is read on every step of the wave-level programs. The kernels keep it in LDS (`hdr` = a __shared__ object of the
// one-wave workgroup): a control-word read is an LDS access instead of an L2 / HBM round trip. hdr == nullptr: at the start of the slab.
RTK_DEV RegionScratch* region_scratch_carve(char* base, const RegionScratchCfg& c, RegionScratch* hdr = nullptr) {
    RegionScratch* s = hdr ? hdr : reinterpret_cast<RegionScratch*>(base);
    char* p = base + ((sizeof(RegionScratch) + 255) / 256 * 256);
    RegionScratch t;
    t.my = scratch_carve(p, c.my); p += scratch_bytes(c.my);
    for (int i = 0; i < RTK_ARENA_N; ++i) { t.arena[i] = p; p += c.arena_cap; t.top[i] = 0; }
    t.arena_cap = c.arena_cap;
    for (int i = 0; i < RTK_L_N; ++i) { t.list[i] = reinterpret_cast<uint64_t*>(p); p += 8ull * c.list_cap; }
    t.list_cap = c.list_cap;
    for (int i = 0; i < RTK_BM_N; ++i) { t.bm[i] = reinterpret_cast<uint64_t*>(p); p += 8ull * c.bm_words; }
    t.bm_words = c.bm_words;
    for (int i = 0; i < RTK_WP_N; ++i) { t.wp[i].ums = reinterpret_cast<UMap*>(p); p += sizeof(UMap) * c.um_cap; t.wp[i].n = 0; t.wp[i].l = 0; t.wp[i].qlen = 0; }
    t.um_cap = c.um_cap;
    for (int i = 0; i < RTK_SET_N; ++i) { t.set[i] = reinterpret_cast<uint32_t*>(p); p += 4ull * c.set_cap; }
    t.set_cap = c.set_cap;
    t.memo_u = reinterpret_cast<uint32_t*>(p); p += 4ull * c.memo_cap; t.memo_cap = c.memo_cap; t.memo_n = 0;
    for (int i = 0; i < RTK_WP_N; ++i) { t.wp[i].qual = p; p += c.str_cap; }
    for (int i = 0; i < RTK_STR_N; ++i) { t.str[i] = p; p += c.str_cap; }
    for (int i = 0; i < RTK_RB_N; ++i) { t.rbuf[i] = p; p += c.str_cap; }
    t.str_cap = c.str_cap;
    t.memo_v = reinterpret_cast<uint8_t*>(p); p += c.memo_cap;
    t.ovf_word = 0; t.overflow = reinterpret_cast<uint32_t*>(&s->ovf_word); t.my.overflow = t.overflow;
    for (int i = 0; i < RTK_RC_N; ++i) t.cnt[i] = 0;
    for (int i = 0; i < RTK_FINE_N; ++i) t.fine[i] = 0;
#ifdef RTK_PROF
    for (int i = 0; i < RTK_LAP_N; ++i) t.prof[i] = 0;
    t.prof_t = rtk_clock();
#endif
#ifndef RTK_SLIM_HDR
    for (int i = 0; i < RTK_H_N; ++i) t.hist[i] = 0;
#endif
    *s = t; // every lane stores the same header
    return s;
}

#endif
