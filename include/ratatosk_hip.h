/*
 * ratatosk_hip.h -- C ABI of the MI355X-native Ratatosk per-long-read correction path.
 *
 * The reference (DecodeGenetics/Ratatosk v0.9.0) has no FFI; its drop-in seam is the body of the
 * per-read worker loop of `Ratatosk correct -1` (reference: src/Ratatosk.cpp:808-864):
 *     getSeeds(opt, dbg, read, qual, false, ~0, m_km_um, false)            src/Graph.hpp:14-18
 *     correctSequence(dbg, opt, read, qual, solid, weak, false, nullptr, ~0, hap_reads, max_km_cov)
 *                                                                           src/Correction.hpp:32-35
 * called on a shared read-only graph loaded by dbg.read() + readGraphData() (src/Ratatosk.cpp:1087-1089,
 * src/Graph.cpp:722). Each entry point below names the reference interface it replaces. Plain pointers
 * and sizes only; every function returns 0 on success and a negative code on failure, with a message
 * available from rtk_last_error() (the reference prints to cerr and exit(1)s; a library must not).
 * All compute runs in HIP kernels on gfx950; there is no CPU fallback: a call fails with
 * RTK_ERR_NO_DEVICE when no GPU/extension is usable.
 */
#ifndef RATATOSK_HIP_H
#define RATATOSK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTK_OK 0
#define RTK_ERR_IO (-1)
#define RTK_ERR_FORMAT (-2)
#define RTK_ERR_ARG (-3)
#define RTK_ERR_NO_DEVICE (-4)
#define RTK_ERR_DEVICE (-5)
#define RTK_ERR_UNSUPPORTED (-6)

typedef struct rtk_graph rtk_graph; /* compacted coloured de Bruijn graph: host image + HBM image */
typedef struct rtk_batch rtk_batch; /* one batch of long reads resident in HBM (reference: the >=1 MiB ticket unit, src/Common.hpp:138) */

/* POD mirror of the Correct_Opt fields read by the pass-1 hot path (reference: src/Common.hpp:101-156). */
typedef struct rtk_opts {
    uint64_t insert_sz;             /* -i, 500  */
    uint64_t min_cov_vertices;      /* 2        */
    uint64_t max_len_weak_region1;  /* -w, 1000 */
    uint64_t max_km_cov;            /* max(getMaxKmerCoverage(dbg,0.001),128), src/Ratatosk.cpp:625 */
    double weak_region_len_factor;  /* 0.25     */
    double large_k_factor;          /* 1.5      */
    double min_score;               /* 0.0 with one correction round, src/Ratatosk.cpp:847 */
    int32_t max_qual;               /* -Q, 40   */
    int32_t out_qual;               /* 1        */
    double min_confidence_snp_corr; /* -m, 0.9 (src/Common.hpp:147): below this confidence a SNP-annotated base is re-decided against the read */
    /* second correction pass (`correct -2`; `long_read_correct` of search(), src/Ratatosk.cpp:618): the graph is coloured by the pass-1
     * reads, the reads' qualities are carried over, regions pass 1 already gave the maximum quality are left alone, no 1-edit search.
     * Needs batches created WITH quality strings. */
    int32_t long_read_correct;      /* 0 = pass 1 */
    int32_t force_unres_snp_corr;   /* -f (src/Ratatosk.cpp:279): second pass only, fixSNPs() (src/Alignment.cpp:846-965) on every read before phasing() (src/Ratatosk.cpp:828) */
    uint64_t max_len_weak_region2;  /* -W, 5000 (src/Common.hpp:110) */
    /* Bifrost assumption [A2] as a switch (the reference calls searchSequence(l_s, false, true, true, true, or_exclusive_match = true),
     * src/Graph.cpp:193, and Bifrost is not in the tree): 0 = every graph k-mer one substitution / insertion / deletion away from a window is
     * reported (union of the three searches); 1 = the searches run substitution -> insertion -> deletion and a window that one of them
     * matched is not searched by the next; 2 = the same in the order insertion -> deletion -> substitution. rtk_opts_default takes it from the
     * environment: RTK_A2_XOR=exclusive (default since round 4: the reading the flag's name asks for) | exclusive-ids | union. */
    int32_t a2_exclusive;
    /* Bifrost assumption [A3] as a switch: the order in which getSuccessors() hands out the (up to four) neighbours of a unitig end, which is the
     * order exploreSubGraph pushes them (src/GraphTraversal.cpp:456-587) and so decides between candidates of equal score. 0 = by the base
     * appended in walk direction, A,C,G,T, on both strands (default); 1 = on the reverse strand by the base as the unitig's own strand spells it
     * (A,C,G,T there = T,G,C,A in walk direction). rtk_opts_default takes it from the environment: RTK_A3_ORDER=walk (default) | strand. */
    int32_t a3_strand_order;
    /* Canonical rule [D1] as a switch. chooseColors visits the anchor colour sets "sorted by cardinality" after iterating an unordered_map keyed by
     * pointers (src/Correction.cpp:286-293: heap addresses + an unstable sort decide the order of sets of EQUAL cardinality); this build orders
     * such ties by unitig id: 0 = ascending (default), 1 = descending. rtk_opts_default takes it from the environment: RTK_D1_ORDER=asc | desc.
     * profiles/r04_d1_count.json counts the reads the choice decides. */
    int32_t d1_desc;
    /* sizeof(rtk_opts) of the library that filled the struct (rtk_opts_default writes it; round 5). Every entry that takes an rtk_opts refuses one whose
     * struct_size is not its own sizeof(rtk_opts) with RTK_ERR_ARG: a caller compiled against an older header (the struct has grown in rounds 2, 3, 4 and 5), or one
     * that zero-fills the struct instead of calling rtk_opts_default, is told so instead of running with fields it never set. New fields go BEFORE this one. */
    uint32_t struct_size;
} rtk_opts;

typedef struct rtk_graph_info {
    uint64_t n_unitigs, n_kmers, n_bases, n_colour_ids, n_global_sets;
    uint64_t table_slots, hbm_bytes;
    uint64_t max_km_cov_top; /* getMaxKmerCoverage(dbg, 0.001), src/Graph.cpp:825-841 */
    int32_t k, device;
} rtk_graph_info;

/* Kernel timing and event counters of the last rtk_batch_run (HIP events on the launch stream). */
typedef struct rtk_stats {
    double ms_total, ms_lookup_exact, ms_mask, ms_lookup_inexact, ms_seeds, ms_regions, ms_correct, ms_stitch;
    uint64_t n_windows, n_probes_exact, n_probes_inexact, n_hits_inexact, n_regions, n_region_items, n_arena_overflow;
    uint64_t n_expand, n_colour_elem, n_path_base, n_align, n_align_cells;
    uint64_t in_bases, out_bases;
    /* wave-cycles (s_memtime ticks summed over all waves) spent by k_regions per phase: colour selection, graph traversal incl.
     * its alignments, consensus + trimming alignments, everything else; and inside those, Myers passes and set algebra */
    uint64_t cyc_colour, cyc_paths, cyc_consensus, cyc_total, cyc_myers, cyc_sets /* path record commit+load */, cyc_tostring, cyc_pathqual;
    /* n_probes_* = k-mer queries (one 8-byte pre-filter word each); n_slots_* = 16-byte table slots visited behind the filter */
    uint64_t n_slots_exact, n_slots_inexact;
    /* traceback walks inside cyc_myers: wave-cycles and alignment moves produced */
    uint64_t cyc_walk, n_moves;
    /* lane-per-region kernel (k_regions_lanes, hip/rtk_region_lane.h; round 5): its time (also part of ms_correct), the regions of its class, and how many of
     * them it handed on to the wave kernel (a capacity, a short-cycle unitig, a character outside A C G T N ...: same results, counted) */
    double ms_lanes;
    uint64_t n_lane_regions, n_lane_handed;
    /* second pass: time of the phasing() step of the ticket, and the reads whose whole-read alignment was skipped because no stretch of theirs was marked
     * (the walk over the CIGAR then returns the corrected read as it is, src/Graph.cpp:975-1069) */
    double ms_phase;
    uint64_t n_phase_skipped;
    /* revision 7: routes of the region program's trims and consensus calls. A trim is read off the last column of one NW sweep of (corrected, raw), stored for
     * the forward strand of a gap region (n_trim_stored) or not (n_trim_column), or made by the SHW distance call (n_trim_fallback: a raw byte other than
     * A C G T, a corrected string above 4096 characters or an empty one). A consensus call takes the alignment of the forward strand's string from the stored
     * sweep of its trim (n_consensus_resumed) or sweeps it anew (n_consensus_swept). A region that skips its second strand (n_strand2_skipped below) counts as
     * resumed: its consensus is decided from that stored sweep alone, without the call. */
    uint64_t n_trim_stored, n_trim_column, n_trim_fallback, n_consensus_resumed, n_consensus_swept;
    /* revision 8: fixAmbiguity's searches for the alleles of linked SNPs, one per decided entry of the safe set. A search can only append for a position whose
     * entry is still undecided; when there is none the search is skipped (n_fa_linked_skipped), else it runs (n_fa_linked_run). n_fa_linked_entries: entries the
     * searches produced. With RTK_FA_LINKED_ALWAYS=1 every search runs; the sum of run and skipped and the entries are the same either way. */
    uint64_t n_fa_linked_run, n_fa_linked_skipped, n_fa_linked_entries;
    /* The second strand of a gap region. A gap region that its forward strand does not settle alone runs the whole correction again on the reverse complement
     * and merges the two (generateConsensus). When the forward result alone decides the bytes (csrc/hip/rtk_region.h, rtk_strand2_skippable)
     * the second strand is skipped (n_strand2_skipped), else it runs (n_strand2_run); the sum is the same under every setting. RTK_STRAND2_ALWAYS=1 runs them all.
     * RTK_STRAND2_AUDIT=1 runs and emits the full route where the rule says skip and counts the regions whose bytes then differ from the forward result
     * (n_strand2_audit_mismatch: 0 unless the rule is wrong). Appended without a new revision number: see RTK_API_REVISION. */
    uint64_t n_strand2_run, n_strand2_skipped, n_strand2_audit_mismatch;
    /* The stored sweep of a gap region's forward trim (n_trim_stored) holds the alignment the consensus would ask for. Its path is walked and parked only where
     * the region goes on to its second strand (n_park_walked); where the second strand is skipped, or the sweep cannot be parked, nobody walks it
     * (n_park_deferred). n_park_walked + n_park_deferred == n_trim_stored; n_moves counts the moves of the walks that were made. RTK_PARK_EAGER=1 walks every
     * sweep that can be parked at the trim, as before. Appended without a new revision number, like the fields above. */
    uint64_t n_park_walked, n_park_deferred;
    /* Revision 10: calls of the region program's colour selection (chooseColors, src/Correction.cpp:215-429; csrc/hip/rtk_region.h, rtk_choose_colors) by the
     * program that answered: the register program (n_colours_small: up to 512 ids on up to 24 side unitigs; n_colours_wide: up to 1664 ids), the bit-vector program in scratch memory (n_colours_bits) or the general program on sorted arrays (n_colours_general).
     * The host simulator has neither of the first two. Calls that ended in an overflow are not counted (their region is redone). RTK_COLOURS_ROUTE=bits skips
     * the register program, RTK_COLOURS_ROUTE=general both bit-vector programs: same selections, same sum. RTK_COLOURS_AUDIT=1 lets the general program repeat
     * every selection another program answered and counts the calls whose two lists differ (n_colours_audit_mismatch: 0 unless a program is wrong); the
     * general program's list is the one used, and n_colour_elem counts the ids of both runs. */
    uint64_t n_colours_small, n_colours_wide, n_colours_bits, n_colours_general, n_colours_audit_mismatch;
    /* The register program sorts the ids of a call once, sizes its bit vectors by the number of distinct ids and keeps them in LDS behind the universe
     * (DESIGN.md §3.2 (h)); n_colours_small / n_colours_wide are its calls with at most / more than 512 ids, repeats counted. A call whose universe and vectors
     * do not fit the LDS buffer is handed on (n_colours_declined_fit) and answered -- and counted -- by one of the other two programs. Appended without a new
     * revision number, like the fields above. */
    uint64_t n_colours_declined_fit;
    /* The forward trim of a gap region keeps only the last column of its sweep, which holds all that the rule of the skip reads (distance, last move). Where the
     * region goes on to its second strand after all, rtk_park_walk sweeps the trimmed string against the raw region a second time, stored, and walks that
     * (n_park_resweeps == n_park_walked then). The second sweep is no alignment of the reference's and is not part of n_align / n_align_cells.
     * RTK_TRIM_STORE=1 stores the table at the trim, as before: 0 second sweeps. Appended without a new revision number, like the fields above. */
    uint64_t n_park_resweeps;
} rtk_stats;

/* dbg.read(G.fasta.gz) + readGraphData(G.rtsk) (reference: src/Ratatosk.cpp:1087-1089; src/Graph.cpp:722-784).
 * Parses the unitig FASTA(.gz) and the .rtsk records, rebuilds the k-mer index (the .bfi file is ignored),
 * flattens everything to SoA/CSR arrays. k must be odd and <= 63: one-word k-mers (k <= 31) serve both passes, two-word k-mers
 * (33 .. 63) the second pass only (long_read_correct = 1; the 1-edit anchor search of the first pass is built on one-word k-mers). */
int rtk_graph_load(const char* unitig_fasta_gz, const char* rtsk, int k, int n_threads, rtk_graph** out);
/* The same with flags. RTK_LOAD_DEVICE_TABLES: the host only parses the two files and packs the unitigs; the lookup structures Bifrost keeps behind
 * find() / getSuccessors() -- the k-mer table with its presence filters, the half-k-mer index of the 1-edit search, the adjacency -- are built in HBM by
 * rtk_graph_upload (hip/rtk_graph_tables.hip; a k-mer that occurs twice in the unitig file is then reported by rtk_graph_upload, RTK_ERR_FORMAT).
 * What `Ratatosk correct` and the Python front end use; rtk_graph_load (flags = 0: everything on the host threads) stays the definition. */
#define RTK_LOAD_DEVICE_TABLES 1u
int rtk_graph_load2(const char* unitig_fasta_gz, const char* rtsk, int k, int n_threads, uint32_t flags, rtk_graph** out);

/* Copies the flat graph into HBM of `device` (HIP device ordinal). Must precede any compute call. */
int rtk_graph_upload(rtk_graph* g, int device);

/* Multi-GPU: rank 0 has loaded the graph; the others create an empty shell with rtk_graph_shell(), every rank
 * exposes its flat buffers so the caller can broadcast them (RCCL over xGMI via torch.distributed), then calls
 * rtk_graph_adopt_device() to mark the HBM image valid. Buffer order is fixed; sizes come from rank 0's info. */
int rtk_graph_shell(int k, rtk_graph** out);
int rtk_graph_n_buffers(const rtk_graph* g);
int rtk_graph_buffer(rtk_graph* g, int idx, void** dev_ptr, uint64_t* bytes);
int rtk_graph_alloc_buffers(rtk_graph* g, int device, const uint64_t* bytes, int n, const rtk_graph_info* info);
int rtk_graph_adopt_device(rtk_graph* g);
/* Same with caller-owned HBM buffers (e.g. torch tensors that torch.distributed broadcasts into); never freed by the library. */
int rtk_graph_attach_buffers(rtk_graph* g, int device, void* const* dev_ptrs, const uint64_t* bytes, int n, const rtk_graph_info* info);
int rtk_graph_buffer_bytes(const rtk_graph* g, uint64_t* bytes, int n);
/* A flat buffer of a resident graph handed over to caller-owned HBM (of at least its rtk_graph_buffer_bytes): copied device to device, the library's own
 * copy freed. For rank 0 of a multi-GPU job whose tables were built by rtk_graph_upload, before it broadcasts them. */
int rtk_graph_move_buffer(rtk_graph* g, int idx, void* dev_ptr, uint64_t bytes);
/* (tests, tools) flat buffer idx of the host image: a pointer into the graph's own memory, valid until rtk_graph_free */
int rtk_graph_host_buffer(const rtk_graph* g, int idx, const void** p, uint64_t* bytes);
/* (tests, tools) `bytes` bytes of flat buffer idx of a resident graph copied to host memory */
int rtk_graph_download_buffer(const rtk_graph* g, int idx, void* host_dst, uint64_t bytes);

/* Single-process multi-GPU (the C++ `Ratatosk correct` driver): the index is parsed and flattened ONCE, uploaded to one GPU and
 * replicated to the others device-to-device (xGMI peer copies, one per flat buffer) -- the reference's worker threads likewise
 * share one graph (src/Ratatosk.cpp:618,727). The clone has no host image; release it with rtk_graph_free. */
int rtk_n_devices(void); /* HIP devices visible to the process (0: every compute call fails with RTK_ERR_NO_DEVICE) */
/* free and total bytes of a device's memory (hipMemGetInfo): a host driver sizes its number of tickets in flight with it */
int rtk_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes);
int rtk_graph_clone_to_device(const rtk_graph* src, int device, rtk_graph** out);

int rtk_graph_get_info(const rtk_graph* g, rtk_graph_info* info);
void rtk_graph_free(rtk_graph* g);
/* Indexes written by the reference carry short-cycle annotations (detectShortCycles, src/Graph.cpp:4660, always) and SNP-ambiguity
 * annotations (detectSNPs, src/Graph.cpp:484, unless -F); both are consumed (fixRepeats, fixAmbiguity). This call drops BOTH kinds
 * from a loaded graph BEFORE rtk_graph_upload, which makes the graph identical to one whose index was written without them.
 * Returns the number of unitigs that carried an annotation, < 0 on error. */
long long rtk_graph_strip_annotations(rtk_graph* g);

/* Optional: allocate the per-wave scratch slabs of the seed and region stages (tens of GB, seconds of hipMalloc) for reads up to
 * max_read_len on `device` ahead of time, e.g. from a helper thread while rtk_graph_load parses the index. The first graph uploaded
 * to that device adopts them. Not part of the reference's seam; there is nothing to release. */
int rtk_reserve_scratch(int device, uint32_t max_read_len);
/* Second pass: n_tickets x (work area of the phasing step, work area of the region stage) reserved ahead; every ticket in flight owns a pair.
 * The first call for a device also reserves the work areas of the per-read seed kernels (one slab per graph). */
int rtk_reserve_second_pass(int device, uint32_t n_tickets, uint64_t phase_bytes, uint64_t region_bytes);
/* Round 6: the device buffers of n_batches tickets of about bases_per_batch bases / reads_per_batch reads (with_qualities: FASTQ input kept, second pass; raw_bases_per_batch != 0: the
 * second pass, which also holds the uncorrected reads) taken from the device and parked in the graph's pool, so that the first tickets of a run find them instead of calling hipMalloc inside the
 * correction phase (a hipMalloc stalls every stream of the device). A batch carves all its arrays out of ONE such buffer. RTK_ERR_DEVICE when an eighth of the device memory would not stay free
 * (what could be reserved stays reserved). */
int rtk_graph_reserve_batches(rtk_graph* g, uint32_t n_batches, uint64_t bases_per_batch, uint32_t reads_per_batch, int with_qualities, uint64_t raw_bases_per_batch);

/* Correct_Opt defaults + max_km_cov derived from the graph (reference: src/Common.hpp:101-156, src/Ratatosk.cpp:625). */
int rtk_opts_default(const rtk_graph* g, rtk_opts* opts);

/* The per-read loop body over one batch (reference: src/Ratatosk.cpp:808-864): upper-casing, quality clamp,
 * getSeeds, correctSequence. Inputs are borrowed; out_seq[i]/out_qual[i] are malloc'd NUL-terminated strings
 * owned by the caller (release with rtk_free). qual may be NULL (FASTA input). */
int rtk_correct_batch(rtk_graph* g, const rtk_opts* opts, uint32_t n, const char* const* seq, const char* const* qual,
                      const uint32_t* len, char** out_seq, char** out_qual, uint32_t* out_len);
/* Revision 6: the tickets of CONCURRENT rtk_correct_batch callers are merged into one launch. The reference's workers each take a ticket of
 * >= 1 MiB of bases (src/Common.hpp:138, src/Ratatosk.cpp:757-772) and call the loop body on it from `-c` threads at once; a launch that small
 * lasts as long as its longest read and leaves the device idle, so a call that arrives while another caller gathers a group joins it (first-pass
 * tickets below RTK_COALESCE_BASES = 16 Mi bases, same rtk_opts bytes, same kind of input; the gatherer waits <= RTK_COALESCE_WAIT_US = 1 500 us
 * when the device idles and another caller has been seen, not at all when it is alone, and for as long as a group in flight has not reached its region stage), the group runs as one batch and every caller copies out its own reads.
 * Results are those of the calls made one by one (reads are independent). RTK_COALESCE_BASES=0 switches it off.
 * rtk_coalesce_stats: groups launched and tickets they held since the graph was loaded (a group of one is a call that ran on its own). */
int rtk_coalesce_stats(rtk_graph* g, uint64_t* n_groups, uint64_t* n_tickets);

/* Same work split so that a caller can keep the batch resident in HBM across the timed region:
 * create = pack + H2D copy, run = kernels only (synchronous), fetch = D2H + unpack. */
int rtk_batch_create(rtk_graph* g, uint32_t n, const char* const* seq, const char* const* qual, const uint32_t* len, rtk_batch** out);
/* Second pass (`correct -2`): the pass-1 corrected reads WITH their qualities plus the uncorrected reads in the same order (the
 * reference reads the two files in lock-step and aborts when the names disagree, src/Ratatosk.cpp:774-802). Run with
 * opts->long_read_correct = 1: phasing() (src/Graph.cpp:869-1097) runs on the device before the seed stage. */
int rtk_batch_create2(rtk_graph* g, uint32_t n, const char* const* seq, const char* const* qual, const uint32_t* len,
                      const char* const* raw, const uint32_t* raw_len, rtk_batch** out);
int rtk_batch_run(rtk_batch* b, const rtk_opts* opts);
/* rtk_batch_run = rtk_batch_run_seeds (getSeeds of every read: src/Graph.cpp:3-482) followed by rtk_batch_run_regions (correctSequence
 * of every read: src/Correction.cpp:159-958). Every batch owns a HIP stream, and each call only waits for that stream: calling the
 * two stages of DIFFERENT batches from two host threads overlaps them on the device (the seed stage is latency-bound and leaves the
 * vector ALUs to the region stage of the previous batch), the way the reference overlaps its worker threads (src/Ratatosk.cpp:727). */
int rtk_batch_run_seeds(rtk_batch* b, const rtk_opts* opts);
int rtk_batch_run_regions(rtk_batch* b, const rtk_opts* opts);
int rtk_batch_fetch(rtk_batch* b, char** out_seq, char** out_qual, uint32_t* out_len);
/* rtk_batch_fetch without the per-read allocations: the corrected records stay packed in (pinned) host memory owned by the batch --
 * read i is pool[off[i] .. +len[i]) followed by its quality string pool[off[i]+len[i] .. +len[i]) -- valid until the batch is freed
 * or run again. What a writer that formats FASTQ blocks needs (reference: writeCorrectedOutput, src/Ratatosk.cpp:510-520). */
int rtk_batch_fetch_view(rtk_batch* b, const char** pool, const uint64_t** off, const uint32_t** len);
int rtk_batch_get_stats(const rtk_batch* b, rtk_stats* stats);
void rtk_batch_free(rtk_batch* b);

/* ---- stage-level entry points (used by the parity tests; same kernels as rtk_batch_run) ---- */

/* dbg.searchSequence(s, true, false, false, false, false) (reference: src/Graph.cpp:97): for every k-mer window p of
 * seq, hits[p] = unitig<<33 | dist<<1 | strand, or -1 when the window is not in the graph / holds a non-ACGT. */
int rtk_lookup_exact(rtk_graph* g, const char* seq, uint32_t len, int64_t* hits);

/* fixSNPs (reference: src/Alignment.cpp:846-965; `-f`, src/Ratatosk.cpp:828) of one read, upper-cased first (src/Ratatosk.cpp:814):
 * out[0..len) = the read with every ambiguous character that has exactly one graph-supported base replaced by it. */
int rtk_fix_snps(rtk_graph* g, const char* seq, uint32_t len, char* out);

/* getSeeds (reference: src/Graph.cpp:3-482): anchors as (pos, unitig, dist, strand) quadruples. */
int rtk_seeds(rtk_graph* g, const rtk_opts* opts, const char* seq, uint32_t len,
              uint64_t* n_solid, int64_t* solid, uint64_t* n_weak, int64_t* weak, uint64_t cap);

/* getSeeds of read `read` of a batch of SEVERAL reads: the anchors rtk_batch_run_seeds left for it, as the same (pos, unitig, dist, strand) quadruples as
 * rtk_seeds, positions in the read's own coordinates (rtk_seeds is this call on a batch of one read). Valid after rtk_batch_run_seeds has completed and
 * until the batch is run again (rtk_batch_run_regions consumes the anchors). *n_solid / *n_weak are the true counts; up to cap quadruples of each list are
 * written. RTK_ERR_ARG for read >= the reads of the batch, for a batch whose seed stage has not completed, and -- after writing what fits, like rtk_seeds --
 * for a cap below either count. Appended without a new revision number: see RTK_API_REVISION. */
int rtk_batch_fetch_seeds(rtk_batch* b, uint32_t read, uint64_t* n_solid, int64_t* solid, uint64_t* n_weak, int64_t* weak, uint64_t cap);

/* edlibAlign + edlibAlignmentToCigar (reference: src/edlib.cpp:141,298) with the IUPAC equality table of
 * src/Common.hpp:262-276 (use_iupac=0: edlibDefaultAlignConfig). mode 0 NW, 1 SHW, 2 HW; k<0 unbounded.
 * dist[i] = editDistance or -1; end_locs holds up to cap_locs locations per problem; cigars (standard format)
 * are written at cigar + i*cap_cigar when want_path. */
int rtk_myers_batch(uint32_t n, const char* const* query, const uint32_t* qlen, const char* const* target, const uint32_t* tlen,
                    const int32_t* k, const int32_t* mode, int want_path, int use_iupac,
                    int32_t* dist, int32_t* n_loc, int32_t* end_locs, uint32_t cap_locs, char* cigar, uint32_t cap_cigar);

/* The same problems on workgroups of `waves` wavefronts (2..16): the schedule the second pass uses for the whole-read alignment of its long
 * reads (reference: phasing(), src/Graph.cpp:975) -- wave 0 runs the alignment program, the others take the row blocks / banded passes it
 * publishes. waves <= 1 is rtk_myers_batch. Stage entry for parity tests and timing of that schedule; same results. */
int rtk_myers_batch_waves(uint32_t n, const char* const* query, const uint32_t* qlen, const char* const* target, const uint32_t* tlen,
                          const int32_t* k, const int32_t* mode, int want_path, int use_iupac,
                          int32_t* dist, int32_t* n_loc, int32_t* end_locs, uint32_t cap_locs, char* cigar, uint32_t cap_cigar, int waves);

/* Test-only modes of rtk_myers_batch (revision 7; one wave per problem, not rtk_myers_batch_waves / _lanes): the routes by which the region program's trim
 * and consensus share one sweep (csrc/hip/rtk_myers_distance.h, rtk_myers_shw_by_column; csrc/hip/rtk_region.h, rtk_trim_by_column).
 *   RTK_MYERS_MODE_SHW_BY_COLUMN: k < 0. The SHW distance of (query, target), read off the last column of ONE NW sweep of (target, query); n_loc = the number
 *     of end locations, of which end_locs holds the first (slot 0) and the last (slot n_loc - 1) only: the route does not list the others. No path.
 *   RTK_MYERS_MODE_NW_PREFIX: 0 <= k <= qlen. The NW distance and, with want_path, the path of (query[0, k), target), walked from row k of the stored NW sweep of
 *     the WHOLE query; end_locs[0] = tlen - 1.
 *   RTK_MYERS_MODE_NW_PREFIX_LAST: 0 <= k <= qlen. The NW distance of (query[0, k), target) and in end_locs[0] the LAST move of the path mode 4 walks (0 match,
 *     1 insert, 2 delete, 3 mismatch), read off the stored sweep without a walk (rtk_myers_last_move: what the deferred park of the forward trim keeps of its
 *     path); -1 where there is no path (k = 0 or an empty target). No path is returned.
 *   RTK_MYERS_MODE_NW_PREFIX_LAST_COLUMN: as mode 5, from a sweep that stores no table: the answer is derived from the delta vectors of the sweep's last
 *     column alone (rtk_myers_last_move_column: what the forward trim of a gap region keeps). Same problems taken, same answers.
 * A problem the route does not take (a target byte other than A C G T -- the sweep's target: the query in mode 3 --, more than 4096 characters in the swept
 * query, a table or move list too big for the in-memory traceback, an empty string) is answered by the calls the route replaces. How the calling thread's last
 * rtk_myers_batch call split its problems of these modes: rtk_myers_column_last_routes (a route that took nothing would pass on the fallback's results). */
#define RTK_MYERS_MODE_SHW_BY_COLUMN 3
#define RTK_MYERS_MODE_NW_PREFIX 4
#define RTK_MYERS_MODE_NW_PREFIX_LAST 5
#define RTK_MYERS_MODE_NW_PREFIX_LAST_COLUMN 6
void rtk_myers_column_last_routes(uint64_t* column_route, uint64_t* fallback);

/* rtk_myers_batch with ONE PROBLEM PER LANE: queries of up to 512 characters against targets of up to 2048 over A, C, G, T, N are computed column by column in a
 * lane's registers, 64 problems per wavefront (csrc/hip/rtk_myers_lane.h); with want_path the lane keeps the delta vectors of its columns (up to 4096
 * word-columns) and walks them back. What does not fit that takes the wave route of rtk_myers_batch. Same results
 * (reference: edlibAlign, src/edlib.cpp:131-296). Stage entry: one alignment per lane as the lane-per-region kernel does them (DESIGN_HISTORY.md section 3.8), for parity tests and
 * timing; the correction path does not call it. */
int rtk_myers_batch_lanes(uint32_t n, const char* const* query, const uint32_t* qlen, const char* const* target, const uint32_t* tlen,
                          const int32_t* k, const int32_t* mode, int want_path, int use_iupac,
                          int32_t* dist, int32_t* n_loc, int32_t* end_locs, uint32_t cap_locs, char* cigar, uint32_t cap_cigar);
/* How the calling thread's last rtk_myers_batch_lanes call split its problems: *lane_route = computed one per lane, *wave_route = handed on to rtk_myers_batch
 * (tests hold the lane route to every problem that fits it: a lane kernel that took nothing would otherwise pass on the wave route's results). */
void rtk_myers_lanes_last_routes(uint64_t* lane_route, uint64_t* wave_route);

/* Index build, device side (the reference builds its index on the CPU: `Ratatosk index`, src/Ratatosk.cpp:1066-1067, Bifrost
 * build + addCoverage src/Graph.cpp:1561). rtk_index_count_kmers: the canonical k-mers (odd k <= 63, A=0 C=1 G=2 T=3, first base in the
 * high bits) that the reads of `files` (plain or gzipped FASTA/FASTQ) hold at least min_count times, sorted ascending; *solid is freed
 * with rtk_free. The tool csrc/tools/build_index.cpp (--gpu) builds the same files with it as its CPU path does.
 * K-mer layout of the index calls: k <= 31 one uint64_t per k-mer; 33 <= k <= 63 TWO uint64_t words per k-mer, low word first (the 2k-bit code
 * as a little-endian unsigned 128-bit integer), in `solid`, `*solid`, `*seeds` and `*left`. Counts (n_solid, n_unitigs, n_left) are in k-mers. */
int rtk_index_count_kmers(int device, int k, const char* const* files, int n_files, uint32_t min_count, int n_threads, uint64_t** solid, uint64_t* n_solid);
/* rtk_index_unitigs: the unitigs of a sorted set of canonical solid k-mers (Bifrost's compaction behind CompactedDBG::build, src/Ratatosk.cpp:1100-1118):
 * the k-mers in a table in HBM with their eight edge bits, every maximal chain of mutually unique links walked from its ends by one thread each, written
 * with its smallest canonical k-mer reading forwards, the unitigs in the order of those k-mers: unitig j = seq_pool[seq_off[j] .. seq_off[j + 1]), seeds[j]
 * its smallest k-mer. Chains that meet themselves (closed loops, hairpins) are not built: their k-mers come back in `left` (sorted) for the caller.
 * Outputs are freed with rtk_free. RTK_ERR_FORMAT if a k-mer ended up on two unitigs (the tool then takes its plain construction). */
int rtk_index_unitigs(int device, int k, const uint64_t* solid, uint64_t n_solid, char** seq_pool, uint64_t** seq_off, uint64_t** seeds, uint64_t* n_unitigs,
                      uint64_t** left, uint64_t* n_left);

/* rtk_index_colour_*: colours and coverage of an index build (addCoverage, src/Graph.cpp:1561-1985: every k-mer of every read mapped onto its unitig).
 * begin: unitig u = seq_pool[seq_off[u] .. seq_off[u + 1]); packs them and builds their k-mer table in HBM. chunk (any thread; calls are serialised inside):
 * sequences separated by '\n', read r starting at starts[r] with the id ids[r] (the caller numbers its reads: a pair keeps one id), at most 64 MB and
 * 4 M reads per call. end: the distinct events unitig << 32 | id in ascending order and the k-mer coverage of every unitig (rtk_free); releases the job
 * (with null outputs: only that). */
int rtk_index_colour_begin(int device, int k, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs, void** job);
int rtk_index_colour_chunk(void* job, const char* chars, uint64_t n_chars, const uint64_t* starts, const uint32_t* ids, uint32_t n_reads);
int rtk_index_colour_end(void* job, uint64_t** events, uint64_t* n_events, uint64_t** cov);
/* rtk_index_colour_chunk with the base-confidence rule of a second-pass index (addCoverage with long_read_correct, src/Graph.cpp:1573, 1806-1814, 1872-1880; DESIGN.md
 * section 4 [A14]): quals runs parallel to chars (quals[i] is the quality byte of chars[i]; the bytes at the '\n' separators are ignored), and a base whose quality byte
 * is below q_min (unsigned comparison; q_min = getQual(min_confidence_2nd_pass, 1, max_qual), src/Common.hpp:410-418) is no base: every k-mer window that holds it gives
 * no event and no coverage, as an 'N' in the sequence does. The characters are rewritten on the device (k_col_mask, on the chunk's stream ahead of the look-up); the
 * caller's buffers are only read. quals == NULL or q_min == 0: exactly rtk_index_colour_chunk. Chunks with and without qualities may follow each other in one job; a job
 * that never sees qualities allocates and launches what it did before this entry existed. The read-length rule of the same block (a read shorter than
 * min_len_2nd_pass colours nothing, src/Graph.cpp:1796, 1870) is the caller's: such reads are not fed, and keep their id. Appended without a new revision number: see
 * RTK_API_REVISION. */
int rtk_index_colour_chunk_q(void* job, const char* chars, const unsigned char* quals, unsigned char q_min, uint64_t n_chars, const uint64_t* starts, const uint32_t* ids,
                             uint32_t n_reads);
/* Colours subsampled by coverage on the device (rtk_build_index --gpu --subsample-colours; the reference: addCoverage, src/Graph.cpp:2312-2870; the rule and its three
 * deviations: DESIGN.md section 4 [A12], csrc/tools/index/subsample.hpp). The caller works out what needs coverage and structure, the device does everything that
 * touches an event or an id, so that only the kept events are copied to the host.
 * rtk_index_colour_cov: finishes the pending chunks and the last sort-and-unique and hands out the k-mer coverage of every unitig (rtk_free); the job stays alive.
 * rtk_index_colour_end_subsampled: bin_of_unitig[u] = the coverage bin of unitig u, 0 .. n_bins - 1 (n_bins <= 64), or 255 for none; forced_candidate[u] = 1 when the
 * unitig is non-branching; bin_is_sampled[j] = 1 when the ids of bin j are drawn. An id belongs to the smallest bin among the unitigs it colours; it is kept when that
 * bin is not sampled, or when u(id) <= rate with u(id) = (h(id) >> 11) * 2^-53, h(id) = the splitmix64 finalizer of id + seed * 0x9E3779B97F4A7C15. Beside that the mcv
 * (<= 64) ids of smallest (h(id), id) of every forced candidate are kept, all of them when it has no more. The kept ids, ascending, are renumbered from 0.
 * *events: the kept events unitig << 32 | new id, ascending and distinct (renumbering is monotone), *n_events of them (rtk_free); *n_events_before = the events before
 * the thinning, *n_ids_before / *n_ids_after = the distinct ids before and after. The job is gone afterwards, also on error. rtk_index_colour_end stays as it is.
 * rtk_index_subsample_events: stage entry for tests -- the same device function on the caller's events (host arrays; ascending, distinct, unitigs < n_unitigs);
 * events_out has room for n_events words. RTK_ERR_NO_DEVICE without a GPU, like every compute entry. */
int rtk_index_colour_cov(void* job, uint64_t** cov);
int rtk_index_colour_end_subsampled(void* job, const uint8_t* bin_of_unitig, const uint8_t* forced_candidate, const uint8_t* bin_is_sampled, uint32_t n_bins, uint32_t mcv,
                                    double rate, uint64_t seed, uint64_t** events, uint64_t* n_events, uint64_t* n_events_before, uint64_t* n_ids_before, uint64_t* n_ids_after);
int rtk_index_subsample_events(int device, const uint64_t* events, uint64_t n_events, uint32_t n_unitigs, const uint8_t* bin_of_unitig, const uint8_t* forced_candidate,
                               const uint8_t* bin_is_sampled, uint32_t n_bins, uint32_t mcv, double rate, uint64_t seed, uint64_t* events_out, uint64_t* n_out,
                               uint64_t* n_ids_before, uint64_t* n_ids_after);
/* Ids of read pairs on the same unitigs merged on the device (rtk_build_index --gpu --merge-duplicates; the reference: "Detecting and removing duplicated reads",
 * src/Graph.cpp:1630-1705 and 2089-2134; the rule and its deviations: DESIGN.md section 4 [A13], csrc/tools/index/merge.hpp). With U(i) the unitigs of id i, g(u) the
 * splitmix64 finalizer of u + 1, S(i) the sum of g over U(i) modulo 2^64 and low(i) = min U(i): ids with equal (S, low) are one class, its leader is its smallest id,
 * the leaders in ascending order are numbered from 0 and every id takes its leader's number. Tables are sized by the ids that have events, never by the largest id.
 * rtk_index_colour_merge: finishes the pending chunks and the last sort-and-unique of an open job, merges its events in place (they stay ascending and distinct) and sets
 * the job's events and ids; the job stays alive, so rtk_index_colour_end, rtk_index_colour_cov and rtk_index_colour_end_subsampled go on from the merged events. Outputs:
 * the events and the distinct ids before and after. rtk_index_colour_merge_classes: what that call found about the classes: how many hold more than one id, and the
 * number of ids of the largest.
 * rtk_index_merge_events: stage entry for tests -- the same device function on the caller's events (host arrays; ascending, distinct, unitigs < n_unitigs); events_out
 * has room for n_events words. RTK_ERR_NO_DEVICE without a GPU, like every compute entry. */
int rtk_index_colour_merge(void* job, uint64_t* n_events_before, uint64_t* n_events_after, uint64_t* n_ids_before, uint64_t* n_ids_after);
int rtk_index_colour_merge_classes(void* job, uint64_t* classes_above_one, uint64_t* largest);
int rtk_index_merge_events(int device, const uint64_t* events, uint64_t n_events, uint32_t n_unitigs, uint64_t* events_out, uint64_t* n_out, uint64_t* n_ids_before,
                           uint64_t* n_ids_after);

/* rtk_index_snp_candidates: the candidate search of the SNP annotations of an index build (rtk_build_index --gpu --snps; detectSNPs, src/Graph.cpp:484-720:
 * searchSequence with one substitution over every window of a unitig) on the device. Unitig u = seq_pool[seq_off[u] .. seq_off[u + 1]) as for rtk_index_colour_begin
 * (characters A/C/G/T, every unitig of at least k of them), odd k in 3 .. 63. searched[u] != 0: the windows of u are queried (NULL: those of every unitig); every
 * unitig, searched or not, is found as a neighbour. For window p of a searched unitig u with the oriented k-mer x, a candidate is a k-mer y that differs from x at
 * exactly one offset j (0 = the first base) with base alt there (A=0 C=1 G=2 T=3) and whose canonical form is a k-mer of a unitig w != u (w == u is what the host rule
 * skips before it looks at anything, src/Graph.cpp:523: dropped here). *cand: two words per candidate, u << 32 | p then j << 40 | alt << 32 | w, ascending by
 * (u, p, j, alt) -- the order in which the host rule visits them; *n_cand of them (rtk_free). A window has at most 3k candidates; no cap drops any.
 * flags & RTK_SNP_FIRST_PER_SITE: of all candidates with equal (u, p + j, alt) only the one with the smallest p is kept, the kept ones again in (u, p, j, alt) order.
 * That is exact for the host's replay: it marks (position p + j, alt) as tried at the first candidate it visits there and returns at once from every later one
 * (`if (seq_tried[at] == ct) return`, csrc/tools/index/annotate.hpp), so only the first in visiting order -- the smallest p -- can have any effect.
 * RTK_ERR_FORMAT when a canonical k-mer occurs twice in the unitigs (or a character is no base). The stage needs two sorted views of the windows of the pool (key + unitig
 * id each), a third such array for the sorts, the sort's temporary, two prefix tables, the counts and offsets of the searched windows, and the candidates; the bytes are
 * worked out before anything is allocated and compared with the room: the free device memory, or RTK_INDEX_SNP_MEM when that is lower. When the views of all windows do
 * not fit, the key space is partitioned: the search runs in P passes, each against views of one range of the keys' leading min(24, 2k) bits (balanced from a histogram of
 * those bits, so that a pass holds about 1/P of the keys), and the candidates of all passes are ordered together at the end -- the same output for every P. P is the
 * smallest number of passes whose plan fits, at most min(256, 2^min(24, 2k)); the environment variable RTK_INDEX_SNP_PASSES (read at the call, 0 or unset: as few as fit)
 * forces exactly that many, clamped to the same cap. RTK_ERR_DEVICE, `need <bytes> bytes of device memory, <room> are to be had`, when not even the most passes fit (or the
 * forced number does not): `need` is the smallest plan -- text, offsets, counts, candidate offsets, tables, temporaries and the views of the smallest partitions --, nothing
 * was allocated, and the caller keeps its host route for that case. Appended without a new revision number: see RTK_API_REVISION.
 * rtk_index_snp_plan: what rtk_index_snp_candidates would do for these unitigs (their offsets are all it needs) with `room` bytes (0: the figure the stage itself would
 * use now), worked out by the same code and without allocating anything. *passes: the number of passes, 0 when nothing fits; *need_one_pass: the bytes of the single pass;
 * *need_min: the bytes of the smallest plan. The figures take every partition at its even share of the keys; the stage, once it has seen the histogram, takes more passes
 * when a partition is heavier than that. */
#define RTK_SNP_FIRST_PER_SITE 1u
int rtk_index_snp_candidates(int device, int k, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* searched, uint32_t flags,
                             uint64_t** cand, uint64_t* n_cand);
int rtk_index_snp_plan(int device, int k, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* searched, uint64_t room, uint32_t* passes,
                       uint64_t* need_one_pass, uint64_t* need_min);

/* rtk_index_pair_ids: the colour ids of the read pairs BY NAME (rtk_build_index --pair-by-name; DESIGN.md section 4 [A18]; the stage: csrc/hip/rtk_index_pairs.h) -- the
 * reference's name_hmap (addCoverage, src/Graph.cpp:1595-1608, 1800-1804): a name gets the next id when it is first seen, every later record of that name the same id.
 * name_hash[r]: the hash of the name of record r of the input, records in input order (the caller hashes: 64-bit FNV-1a over the name, then the mixer of the k-mer
 * tables, csrc/common/name_hash.hpp; two names are the same when their hashes are). ids[r] (room for n words, the caller's) = the number of distinct hashes whose first
 * record precedes the first record of hash name_hash[r]; *n_ids = the number of distinct hashes. n = 0: RTK_OK and nothing written; n >= 2^32: RTK_ERR_UNSUPPORTED
 * before anything is allocated. The stage sorts (hash, ordinal), marks the first of every run and ranks the firsts; the bytes are worked out before anything is allocated
 * and compared with the room: the free device memory, or RTK_INDEX_PAIR_MEM when that is lower. When the sort's buffers for all records do not fit, the hash space is cut
 * into P equal ranges and the stage runs in P passes, each over the records of one range in their input order (the hashes stay on the host and are streamed through
 * a staging buffer every pass); 4 bytes per record live across the passes. P is the smallest number whose plan fits, at most 256; RTK_INDEX_PAIR_PASSES (read at the call,
 * 0 or unset: as few as fit) forces exactly that many, clamped to 256. The same ids for every P. RTK_ERR_DEVICE, `need <bytes> bytes of device memory, <room> are to be
 * had`, when not even the most passes fit (or the forced number does not): the caller keeps its host route for that case. Appended without a new revision number: see
 * RTK_API_REVISION.
 * rtk_index_pair_plan: what rtk_index_pair_ids would do for n records with `room` bytes (0: the figure the stage itself would use now), worked out by the same code and
 * without allocating anything. *passes: the number of passes, 0 when nothing fits; *need_one_pass: the bytes of the single pass; *need_min: the bytes of the smallest plan.
 * The figures take every pass at its even share of the records; the stage, once it has counted them, takes more passes when a range is heavier than that. */
int rtk_index_pair_ids(int device, const uint64_t* name_hash, uint64_t n, uint32_t* ids, uint64_t* n_ids);
int rtk_index_pair_plan(int device, uint64_t n, uint64_t room, uint32_t* passes, uint64_t* need_one_pass, uint64_t* need_min);

/* rtk_index_cover_*: where the text of other sequences (the unitigs of the k2 graph) crosses an edge of these unitigs that too few colours share -- the search of
 * the last block of the reference's first-pass addCoverage, "Covering low coverage edges." (src/Graph.cpp:3085-3363; DESIGN.md section 4 [A16]; the stage:
 * csrc/hip/rtk_index_cover.h). Any odd k <= 63.
 * begin: the unitigs as for rtk_index_colour_begin (packed, with their k-mer table in HBM), at most 2^30 of them (RTK_ERR_UNSUPPORTED above); low_bits[u]: the
 * recorded edges of unitig u -- bit 1, 2, 4, 8 for the successor of its forward strand that appends A, C, G, T, the same bits << 4 for the successors of its
 * reverse strand. chunk (calls are serialised): pieces of sequences separated by '\n', n_chars characters (at most 64 MB and 4 M pieces per call); piece r starts at
 * starts[r] (starts[0] = 0, ascending), belongs to sequence seq_numbers[r] and begins at position first_positions[r] of that sequence. A sequence longer than a chunk
 * is cut by the caller so that every k + 1 consecutive characters lie whole inside exactly one piece (a piece starts k characters before the end of the one before);
 * a sequence of more than 2^32 characters is refused (RTK_ERR_UNSUPPORTED). end: the crossings of all chunks, two words each, ascending by the first word -- the order
 * of the sequence numbers, left to right inside a sequence --, *n of them (rtk_free); releases the job (also on error; with null outputs: only that).
 * A crossing: position p of a sequence where the k characters at p and at p + 1 are all A/C/G/T (either case), the k-mer at p is the last k-mer of its unitig u in
 * the direction the text walks it, the k-mer at p + 1 lies in the graph (on unitig v, which may be u), and the recorded bit of u for that direction and character
 * p + k is set. word 0 = sequence number << 32 | p; word 1 = u << 33 | v << 3 | direction << 2 | base (direction 1: u walked on its reverse strand; base: A=0 .. T=3
 * of character p + k). The bits are only read: testing, clearing and handing out ids in order is the caller's. The capacity of the survivor buffer is counted
 * (RTK_INDEX_COVER_CAP, default 2^20 crossings): a chunk that finds more is mapped a second time into a larger one. Appended without a new revision number: see
 * RTK_API_REVISION. */
int rtk_index_cover_begin(int device, int k, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* low_bits, void** job);
int rtk_index_cover_chunk(void* job, const char* chars, uint64_t n_chars, const uint64_t* starts, const uint32_t* seq_numbers, const uint64_t* first_positions, uint32_t n_seqs);
int rtk_index_cover_end(void* job, uint64_t** crossings, uint64_t* n);

/* rtk_rescue_*: the rescue of unmapped short reads before the index build (`correct -u`; retrieveMissingReads, src/Graph.cpp:3857-4131, called at
 * src/Ratatosk.cpp:1040-1056), with exact sets where the reference has Bloom filters ([A11]). One-word k-mers (odd k <= 31).
 * begin (replaces buildBBF + the long-read graph build, src/Graph.cpp:3880-3884): lr / sr = the canonical k-mers seen at least twice in the long reads / in
 * the `-s` reads, sorted ascending and distinct, as rtk_index_count_kmers(min_count = 2) returns them (either may be empty). D = lr \ sr is formed on the device
 * and put into a table in HBM; the inputs are not kept. chunk (replaces the query loop, src/Graph.cpp:3998-4015; any thread, two calls run side by side):
 * sequences separated by '\n' as for rtk_index_colour_chunk (read r starts at starts[r]; at most 64 MB and 4 M reads per call); keep[r] = 1 when read r has at
 * least min_positions start positions whose k characters are all A/C/G/T (either case) and spell a k-mer of D (positions are counted, not distinct k-mers:
 * src/Graph.cpp:4045), else 0. end: the positions that probed D (all-A/C/G/T windows) and those that hit, over all chunks; releases the job (with null
 * outputs: only that). */
int rtk_rescue_begin(int device, int k, const uint64_t* lr, uint64_t n_lr, const uint64_t* sr, uint64_t n_sr, uint32_t min_positions, void** job);
int rtk_rescue_chunk(void* job, const char* chars, uint64_t n_chars, const uint64_t* starts, uint32_t n_reads, unsigned char* keep);
int rtk_rescue_end(void* job, uint64_t* n_positions_probed, uint64_t* n_hits);

/* rtk_qv_*: the k-mer QV of reads against a set of k-mers (rtk_qv, `correct --qv`; DESIGN.md section 4, [A17]; no counterpart in the reference). One-word k-mers
 * (odd k <= 31). begin: solid = canonical k-mers, sorted ascending and distinct, as rtk_index_count_kmers returns them (may be empty: nothing is ever found); they
 * are put into a table in HBM, the input is not kept. chunk (any thread, two calls run side by side): pieces separated by '\n' as for rtk_rescue_chunk, piece p =
 * chars[starts[p] .. starts[p + 1]) (starts[0] = 0, ascending; the last piece ends at n_chars; at most 64 MB and 4 M pieces per call); windows[p] = the start
 * positions of piece p whose k characters are all A/C/G/T (either case), found[p] = those whose canonical k-mer is in the set. A window that holds the separator
 * or any other character is not valid, so the text alone decides and no window reaches into the next piece. A piece is a whole read or part of one: a read longer
 * than a chunk is cut by the caller with an overlap of k - 1 characters, so that every window lies whole in exactly one piece, and the caller adds the pieces up.
 * The device cuts the work by position (spans of rtk_qv_span() start positions), not by piece: no read sets the launch time. end: valid windows and found ones
 * over all chunks; releases the job (also on error; with null outputs: only that). Appended without a new revision number: see RTK_API_REVISION. */
int rtk_qv_begin(int device, int k, const uint64_t* solid, uint64_t n_solid, void** job);
int rtk_qv_chunk(void* job, const char* chars, uint64_t n_chars, const uint64_t* starts, uint32_t n_pieces, uint32_t* windows, uint32_t* found);
int rtk_qv_end(void* job, uint64_t* n_windows, uint64_t* n_found);
uint32_t rtk_qv_span(void); /* start positions one wave takes at a time (for tests) */

/* rtk_identity_*: the identity of reads to their simulated truth (rtk_identity, `correct --truth-ref --truth-tsv`; DESIGN.md section 4, [A19]; no counterpart in
 * the reference). begin: record r of the reference = ref[rec_off[r] .. rec_off[r + 1]) (rec_off[0] = 0, ascending, n_rec + 1 entries), already upper-cased; the
 * text is copied to HBM once and the input is not kept. max_len = the longest read or stretch a chunk may hold: it sizes the per-wave work areas; if reference,
 * work areas and chunk buffers do not fit the free device memory the error names both byte counts. chunk (any thread, two calls run side by side): reads
 * separated by '\n' in the layout of rtk_qv_chunk (read i = chars[starts[i] .. starts[i + 1] - 1), the last one ends at n_chars - 1; at most 64 MB and 4 M reads
 * per call); the truth of read i is the stretch [t_start[i], t_start[i] + t_len[i]) of record rec[i], reversed and complemented (A<->T, C<->G, any other byte as
 * it is) when rev[i] != 0 -- cut on the device from the resident reference. dist[i] = the exact unit-cost NW edit distance of read i and its truth, bytes equal
 * iff identical (no IUPAC table, no cap). RTK_ERR_ARG, before anything is launched, for a stretch outside its record or a length above max_len. end: the number
 * of pairs and the distance sum over all chunks; releases the job (also on error; with null outputs: only that). Appended without a new revision number: see
 * RTK_API_REVISION. */
int rtk_identity_begin(int device, const char* ref, uint64_t n_ref, const uint64_t* rec_off, uint32_t n_rec, uint32_t max_len, void** job);
int rtk_identity_chunk(void* job, const char* chars, uint64_t n_chars, const uint64_t* starts, uint32_t n_reads,
                       const uint32_t* rec, const uint64_t* t_start, const uint32_t* t_len, const unsigned char* rev, int32_t* dist);
int rtk_identity_end(void* job, uint64_t* n_pairs, uint64_t* sum_dist);

/* Stage entry for tests (revision 10): the wave-cooperative set primitives of the region stage (csrc/hip/rtk_sets.h, rtk_colours.h), one problem per wavefront
 * in ONE launch, each wave with the LDS buffer to itself as in the region kernel. Problem i: the operation op[i], two arrays of 32-bit words a[i][0 .. na[i]) and
 * b[i][0 .. nb[i]) and scalar[i]; its output words go to out_pool[out_off[i] .. out_off[i + 1]) (the caller sizes the slices), out_n[i] says how many were
 * written, result[i] holds the operation's scalar result, status[i] is RTK_SETS_OK or RTK_SETS_NOT_IN_BUILD (the operation has no version in this build: the
 * host simulator has no radix sorts and no 8-lane vectors). RTK_ERR_ARG when a problem breaks a limit below or its slice is too small.
 *   UNION, INTER, DIFF: a and b sorted ascending without repeats; out = a | b (slice >= na + nb), a & b, a \ b (slice >= na); result = out_n.
 *   INTER_COUNT: result = |a & b| counted up to the cap scalar (the count may stop anywhere at or above the cap); no output words.
 *   SORT_PAIRS: na pairs, a = the 64-bit keys and b = the 64-bit values as (low word, high word) each, nb = na; out = the na keys then the na values, in
 *     ascending (key, value) order (slice >= 4 na). A pair of two all-ones words cannot be told from the padding.
 *   RADIX_U32: na <= 1664 keys <= scalar; out = the keys ascending. Keys and counters lie in LDS as the colour selection lays them out: up to 512 keys with the
 *     second buffer in LDS too, above that -- or whenever nb != 0 -- the wide layout with the second buffer in device memory.
 *   RADIX_PAIRS_U32: a = na keys <= scalar, b = their payloads (nb = na); out = keys then payloads, stable ascending by key (slice >= 2 na).
 *   BM_LOWEST: a = a universe of na <= 4096 ids (sorted, no repeats), b = nb ids of it (sorted, no repeats); the bit vector of b over the universe
 *     (rtk_bm_from_ids), result = its population count, out = the ids of its scalar lowest bits (slice >= min(scalar, nb)).
 *   BM8_LOWEST: the same with the vector in lanes 0 .. 7 (rtk_bm8_lowest, rtk_bm8_count): na <= 512.
 *   RADIX_TAGGED: the universe sort of the register program (rtk_radix_sort_tagged in the layout of rtk_colour_universe, rtk_colours.h): a = na <= 1664 ids <= scalar
 *     <= 0xFFFFFFFE, b = their tags < 48 (nb = na); out = ids then tags, stable ascending by id (slice >= 2 na). The scalar chooses the form as the largest id of a
 *     call does: below 2^26 the tag rides in the low bits of the id's word, from there on in a byte array beside it. Device only.
 *   COLOUR_UNIVERSE: universe and bit vectors of the register program (rtk_colour_universe): a = the ids of nb <= 48 lists one after the other (na <= 1664 in
 *     all, each list sorted without repeats or not: only membership counts), b = the nb list lengths, scalar as for RADIX_TAGGED. out = U, VW, the U distinct
 *     ids ascending, then nb vectors of VW 64-bit words (low word, high word): bit r of vector t is set when list t holds the id of rank r
 *     (slice >= 2 + na + 2 nb max(1, ceil(na / 64))); result = U. status RTK_SETS_DECLINED and no output words when universe and vectors do not fit the LDS buffer
 *     the way the register program lays them out. Device only. */
#define RTK_SETS_UNION 0
#define RTK_SETS_INTER 1
#define RTK_SETS_DIFF 2
#define RTK_SETS_INTER_COUNT 3
#define RTK_SETS_SORT_PAIRS 4
#define RTK_SETS_RADIX_U32 5
#define RTK_SETS_RADIX_PAIRS_U32 6
#define RTK_SETS_BM_LOWEST 7
#define RTK_SETS_BM8_LOWEST 8
#define RTK_SETS_RADIX_TAGGED 9
#define RTK_SETS_COLOUR_UNIVERSE 10
#define RTK_SETS_OK 0
#define RTK_SETS_NOT_IN_BUILD 1
#define RTK_SETS_DECLINED 2
int rtk_sets_batch(uint32_t n, const uint32_t* op, const uint32_t* const* a, const uint32_t* na, const uint32_t* const* b, const uint32_t* nb, const uint32_t* scalar,
                   uint32_t* out_pool, const uint64_t* out_off, uint32_t* out_n, uint32_t* result, uint32_t* status);

void rtk_free(void* p);
/* rtk_free of p[0 .. n) (the out_seq / out_qual arrays of rtk_correct_batch in one call; entries are set to NULL). */
void rtk_free_many(void** p, uint32_t n);
const char* rtk_last_error(void);
const char* rtk_version(void);
/* Interface revision, raised whenever a struct of this header grows or a default changes (5: rtk_opts.struct_size, rtk_stats lane fields, a2_exclusive default 1;
 * 7: rtk_stats route fields n_trim_* / n_consensus_*, the test-only rtk_myers_batch modes 3 and 4, rtk_myers_column_last_routes;
 * 8: rtk_stats fields n_fa_linked_*; 9: rtk_rescue_begin / _chunk / _end; still 9: rtk_stats fields n_strand2_* and n_park_*, the test-only rtk_myers_batch mode 5, appended at the end -- a library of revision 9
 * without them leaves them as the caller set them;
 * 10: rtk_sets_batch, rtk_stats fields n_colours_*; still 10: rtk_index_colour_cov, rtk_index_colour_end_subsampled, rtk_index_subsample_events, then rtk_index_colour_merge,
 * rtk_index_colour_merge_classes, rtk_index_merge_events, then rtk_index_colour_chunk_q, then rtk_batch_fetch_seeds, then rtk_index_snp_candidates, then rtk_index_snp_plan, then rtk_index_cover_begin / _chunk / _end, then rtk_qv_begin / _chunk / _end / _span, then rtk_index_pair_ids / rtk_index_pair_plan, then rtk_identity_begin / _chunk / _end, appended -- a library of revision 10 without them lacks the symbols, and callers look them up by name;
 * then the rtk_stats field n_park_resweeps and the test-only rtk_myers_batch mode 6, which are no symbols: a library of revision 10 without them leaves the field as the
 * caller set it and answers mode 6 with RTK_ERR_ARG). */
#define RTK_API_REVISION 10
int rtk_api_revision(void);

#ifdef __cplusplus
}
#endif

#endif /* RATATOSK_HIP_H */
