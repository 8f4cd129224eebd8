"""Python host side over the C ABI of libratatosk_hip.so (include/ratatosk_hip.h).

Mirrors the reference's per-read seam (reference: src/Ratatosk.cpp:808-864 -- getSeeds + correctSequence on a
shared read-only graph) with the same option names as Correct_Opt (src/Common.hpp:101-156). All compute happens
in the HIP kernels; this module only marshals pointers. There is no CPU fallback: a missing extension or a
missing GPU raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTK_LIB_OVERRIDE") or os.path.join(_HERE, "libratatosk_hip.so")  # the override is for A/B runs of two builds (profiles/scripts/ab_lib.sh)


class RtkError(RuntimeError):
    pass


class RtkOpts(C.Structure):
    _fields_ = [("insert_sz", C.c_uint64), ("min_cov_vertices", C.c_uint64), ("max_len_weak_region1", C.c_uint64),
                ("max_km_cov", C.c_uint64), ("weak_region_len_factor", C.c_double), ("large_k_factor", C.c_double),
                ("min_score", C.c_double), ("max_qual", C.c_int32), ("out_qual", C.c_int32), ("min_confidence_snp_corr", C.c_double),
                ("long_read_correct", C.c_int32), ("force_unres_snp_corr", C.c_int32), ("max_len_weak_region2", C.c_uint64),
                ("a2_exclusive", C.c_int32), ("a3_strand_order", C.c_int32), ("d1_desc", C.c_int32), ("struct_size", C.c_uint32)]


class RtkGraphInfo(C.Structure):
    _fields_ = [("n_unitigs", C.c_uint64), ("n_kmers", C.c_uint64), ("n_bases", C.c_uint64), ("n_colour_ids", C.c_uint64),
                ("n_global_sets", C.c_uint64), ("table_slots", C.c_uint64), ("hbm_bytes", C.c_uint64), ("max_km_cov_top", C.c_uint64),
                ("k", C.c_int32), ("device", C.c_int32)]


class RtkStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("ms_total", "ms_lookup_exact", "ms_mask", "ms_lookup_inexact", "ms_seeds", "ms_regions", "ms_correct", "ms_stitch")] + \
               [(n, C.c_uint64) for n in ("n_windows", "n_probes_exact", "n_probes_inexact", "n_hits_inexact", "n_regions", "n_region_items", "n_arena_overflow",
                                         "n_expand", "n_colour_elem", "n_path_base", "n_align", "n_align_cells", "in_bases", "out_bases",
                                         "cyc_colour", "cyc_paths", "cyc_consensus", "cyc_total", "cyc_myers", "cyc_sets", "cyc_tostring", "cyc_pathqual", "n_slots_exact", "n_slots_inexact", "cyc_walk", "n_moves")] + \
               [("ms_lanes", C.c_double), ("n_lane_regions", C.c_uint64), ("n_lane_handed", C.c_uint64), ("ms_phase", C.c_double), ("n_phase_skipped", C.c_uint64)] + \
               [(n, C.c_uint64) for n in ("n_trim_stored", "n_trim_column", "n_trim_fallback", "n_consensus_resumed", "n_consensus_swept",
                                         "n_fa_linked_run", "n_fa_linked_skipped", "n_fa_linked_entries",
                                         "n_strand2_run", "n_strand2_skipped", "n_strand2_audit_mismatch",
                                         "n_park_walked", "n_park_deferred",
                                         "n_colours_small", "n_colours_wide", "n_colours_bits", "n_colours_general", "n_colours_audit_mismatch", "n_colours_declined_fit",
                                         "n_park_resweeps")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


_libs = {}


# kernels of several tickets / streams only run side by side if the HIP runtime may open enough hardware queues (default 4 per process);
# read when the runtime initialises, so it is set before the library is loaded (and only if the caller has not chosen a value)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")


def load_library(path=None):
    """dlopen the extension; fails loudly when it has not been built (no silent fallback)."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RtkError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` (make -C ratatosk_amd/csrc)" % path)
    L = C.CDLL(path)
    L.rtk_last_error.restype = C.c_char_p
    L.rtk_version.restype = C.c_char_p
    L.rtk_graph_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.rtk_graph_load2.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.rtk_graph_move_buffer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
    L.rtk_graph_host_buffer.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.rtk_graph_download_buffer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]
    L.rtk_graph_upload.argtypes = [C.c_void_p, C.c_int]
    L.rtk_graph_shell.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.rtk_graph_n_buffers.argtypes = [C.c_void_p]
    L.rtk_graph_buffer.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.rtk_graph_alloc_buffers.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_int, C.POINTER(RtkGraphInfo)]
    L.rtk_graph_adopt_device.argtypes = [C.c_void_p]
    L.rtk_graph_buffer_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    L.rtk_graph_get_info.argtypes = [C.c_void_p, C.POINTER(RtkGraphInfo)]
    L.rtk_graph_free.argtypes = [C.c_void_p]
    L.rtk_opts_default.argtypes = [C.c_void_p, C.POINTER(RtkOpts)]
    L.rtk_correct_batch.argtypes = [C.c_void_p, C.POINTER(RtkOpts), C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    L.rtk_batch_create.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)]
    L.rtk_batch_create2.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)]
    L.rtk_batch_run.argtypes = [C.c_void_p, C.POINTER(RtkOpts)]
    L.rtk_graph_strip_annotations.restype = C.c_longlong
    L.rtk_graph_strip_annotations.argtypes = [C.c_void_p]
    L.rtk_batch_run_seeds.argtypes = [C.c_void_p, C.POINTER(RtkOpts)]
    L.rtk_batch_run_regions.argtypes = [C.c_void_p, C.POINTER(RtkOpts)]
    L.rtk_batch_fetch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    L.rtk_batch_fetch_view.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint32))]
    L.rtk_n_devices.restype = C.c_int
    L.rtk_device_memory.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.rtk_graph_clone_to_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.rtk_batch_get_stats.argtypes = [C.c_void_p, C.POINTER(RtkStats)]
    L.rtk_batch_free.argtypes = [C.c_void_p]
    L.rtk_lookup_exact.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_int64)]
    L.rtk_fix_snps.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p]
    L.rtk_seeds.argtypes = [C.c_void_p, C.POINTER(RtkOpts), C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_int64),
                            C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.c_uint64]
    L.rtk_myers_batch.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_char_p), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.c_char_p, C.c_uint32]
    L.rtk_myers_batch_waves.argtypes = L.rtk_myers_batch.argtypes + [C.c_int]
    L.rtk_myers_batch_lanes.argtypes = L.rtk_myers_batch.argtypes
    L.rtk_myers_batch_lanes.restype = C.c_int
    L.rtk_coalesce_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.rtk_graph_reserve_batches.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_uint64]
    L.rtk_free_many.argtypes = [C.POINTER(C.c_void_p), C.c_uint32]; L.rtk_free_many.restype = None
    if L.rtk_api_revision() >= 9:  # (an older build given as RTK_LIB_OVERRIDE has no rescue entries: rescue_reads says so)
        L.rtk_rescue_begin.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
        L.rtk_rescue_chunk.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_ubyte)]
        L.rtk_rescue_end.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if L.rtk_api_revision() >= 10:  # (an older build has no rtk_sets_batch: sets_batch says so)
        L.rtk_sets_batch.argtypes = [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    if hasattr(L, "rtk_index_subsample_events"):  # (still revision 10: appended; a library without them: index_subsample_events says so)
        L.rtk_index_colour_cov.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64))]
        L.rtk_index_colour_end_subsampled.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.c_uint32, C.c_uint32, C.c_double, C.c_uint64,
                                                      C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.rtk_index_subsample_events.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint32, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte), C.c_uint32, C.c_uint32,
                                                 C.c_double, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if hasattr(L, "rtk_index_merge_events"):  # (still revision 10: appended; a library without them: index_merge_events says so)
        L.rtk_index_colour_merge.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.rtk_index_colour_merge_classes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.rtk_index_merge_events.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if hasattr(L, "rtk_index_colour_chunk_q"):  # (still revision 10: appended; a library without it: index_colour_reads says so)
        L.rtk_index_colour_chunk_q.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_ubyte, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_uint32]
    if hasattr(L, "rtk_batch_fetch_seeds"):  # (still revision 10: appended; a library without it: Batch.seeds says so)
        L.rtk_batch_fetch_seeds.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.c_uint64]
    if hasattr(L, "rtk_index_snp_candidates"):  # (still revision 10: appended; a library without it: index_snp_candidates says so)
        L.rtk_index_snp_candidates.argtypes = [C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_ubyte), C.c_uint32,
                                               C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]
    if hasattr(L, "rtk_index_snp_plan"):  # (still revision 10: appended; a library without it: index_snp_plan says so)
        L.rtk_index_snp_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_ubyte), C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64)]
    if hasattr(L, "rtk_index_cover_begin"):  # (still revision 10: appended; a library without them: index_cover_crossings says so)
        L.rtk_index_cover_begin.argtypes = [C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_ubyte), C.POINTER(C.c_void_p)]
        L.rtk_index_cover_chunk.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_uint32]
        L.rtk_index_cover_end.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]
    if hasattr(L, "rtk_qv_begin"):  # (still revision 10: appended; a library without them: qv_reads says so)
        L.rtk_qv_begin.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_void_p)]
        L.rtk_qv_chunk.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.rtk_qv_end.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.rtk_qv_span.argtypes = []; L.rtk_qv_span.restype = C.c_uint32
    if hasattr(L, "rtk_identity_begin"):  # (still revision 10: appended; a library without them: identity_reads says so)
        L.rtk_identity_begin.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        L.rtk_identity_chunk.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_ubyte), C.POINTER(C.c_int32)]
        L.rtk_identity_end.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if hasattr(L, "rtk_index_pair_ids"):  # (still revision 10: appended; a library without them: index_pair_ids / index_pair_plan say so)
        L.rtk_index_pair_ids.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.rtk_index_pair_plan.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.rtk_free.argtypes = [C.c_void_p]
    _libs[path] = L
    return L


RTK_LOAD_DEVICE_TABLES = 1


def _b(s):
    return s.encode() if isinstance(s, str) else s


class Graph:
    """The compacted coloured de Bruijn graph, loaded from the reference's index files and resident in HBM."""

    def __init__(self, fasta_gz, rtsk, k=31, device=0, lib_path=None, upload=True, n_threads=None, host_tables=None):
        """host_tables: build the lookup structures (k-mer table, half-k-mer index, adjacency) on the host threads instead of in HBM at upload time.
        Default: on the device whenever the graph is uploaded (RTK_LOAD_DEVICE_TABLES); a graph that stays on the host (upload=False) gets the host's."""
        self.L = load_library(lib_path)
        self.h = C.c_void_p()
        if n_threads is None:  # parse + flatten on the host's threads (same image whatever their number)
            n_threads = max(1, min(32, os.cpu_count() or 1))
        if host_tables is None:
            host_tables = not upload or os.environ.get("RTK_HOST_TABLES") == "1"
        self._check(self.L.rtk_graph_load2(_b(fasta_gz), _b(rtsk), k, n_threads, 0 if host_tables else RTK_LOAD_DEVICE_TABLES, C.byref(self.h)))
        self.k = k
        if upload:
            self._check(self.L.rtk_graph_upload(self.h, device))

    def _check(self, rc):
        if rc != 0:
            raise RtkError("rtk error %d: %s" % (rc, self.L.rtk_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.rtk_graph_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        i = RtkGraphInfo()
        self._check(self.L.rtk_graph_get_info(self.h, C.byref(i)))
        return i

    def opts(self, **kw):
        o = RtkOpts()
        self._check(self.L.rtk_opts_default(self.h, C.byref(o)))
        for k_, v in kw.items():
            setattr(o, k_, v)
        return o

    def lookup_exact(self, seq):
        s = _b(seq)
        nw = max(0, len(s) - self.k + 1)
        out = (C.c_int64 * max(1, nw))()
        self._check(self.L.rtk_lookup_exact(self.h, s, len(s), out))
        return [out[i] for i in range(nw)]

    def fix_snps(self, seq):
        """fixSNPs() of one read (`-f` of the second pass, src/Alignment.cpp:846-965)."""
        s = _b(seq)
        out = C.create_string_buffer(len(s) + 1)
        self._check(self.L.rtk_fix_snps(self.h, s, len(s), out))
        return out.raw[:len(s)]

    def seeds(self, seq, opts=None):
        s = _b(seq)
        o = opts or self.opts()
        cap = 64 * len(s) + 64
        ns, nw = C.c_uint64(), C.c_uint64()
        so, we = (C.c_int64 * (4 * cap))(), (C.c_int64 * (4 * cap))()
        self._check(self.L.rtk_seeds(self.h, C.byref(o), s, len(s), C.byref(ns), so, C.byref(nw), we, cap))
        f = lambda a, n: [(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]) for i in range(n)]
        return f(so, ns.value), f(we, nw.value)

    def correct_batch(self, seqs, quals=None, opts=None, raw=None):
        """[(corrected seq, corrected qual)] for a batch of long reads (one call == one ticket batch).
        Second pass: opts.long_read_correct = 1, quals = the pass-1 qualities, raw = the uncorrected reads (same order)."""
        b = Batch(self, seqs, quals, raw)
        try:
            b.run(opts)
            return b.fetch()
        finally:
            b.close()


class Batch:
    """A batch of long reads resident in HBM: create (H2D) / run (kernels) / fetch (D2H)."""

    def __init__(self, graph, seqs, quals=None, raw=None):
        self.g = graph
        self.L = graph.L
        n = len(seqs)
        bs = [_b(s) for s in seqs]
        seq_arr = (C.c_char_p * n)(*bs)
        qual_arr = None
        if quals is not None:
            bq = [_b(q) for q in quals]
            qual_arr = (C.c_char_p * n)(*bq)
        lens = (C.c_uint32 * n)(*[len(b) for b in bs])
        self.n = n
        self.lens = [len(b) for b in bs]
        self.in_bases = sum(self.lens)
        self.h = C.c_void_p()
        if raw is not None:
            br = [_b(s) for s in raw]
            raw_arr = (C.c_char_p * n)(*br)
            raw_lens = (C.c_uint32 * n)(*[len(b) for b in br])
            graph._check(self.L.rtk_batch_create2(graph.h, n, seq_arr, qual_arr, lens, raw_arr, raw_lens, C.byref(self.h)))
        else:
            graph._check(self.L.rtk_batch_create(graph.h, n, seq_arr, qual_arr, lens, C.byref(self.h)))

    def run(self, opts=None):
        o = opts or self.g.opts()
        self.g._check(self.L.rtk_batch_run(self.h, C.byref(o)))

    def run_seeds(self, opts=None):
        """Stage A (anchors). May run on another host thread while run_regions of a different batch is in flight."""
        o = opts or self.g.opts()
        self.g._check(self.L.rtk_batch_run_seeds(self.h, C.byref(o)))

    def run_regions(self, opts=None):
        """Stage B (region correction + stitching); needs run_seeds of this batch."""
        o = opts or self.g.opts()
        self.g._check(self.L.rtk_batch_run_regions(self.h, C.byref(o)))

    def seeds(self, i, cap=None):
        """Anchors of read i after run_seeds, as Graph.seeds gives them for a single read: (solid, weak) lists of (pos, unitig, dist, strand) with positions
        in the read's own coordinates (stage entry rtk_batch_fetch_seeds). Valid until the batch is run again."""
        if not hasattr(self.L, "rtk_batch_fetch_seeds"):
            raise RtkError("%s lacks rtk_batch_fetch_seeds (anchors of one read of a batch: appended at interface revision 10)" % self.L._name)
        ns, nw = C.c_uint64(), C.c_uint64()
        if cap is None:  # ask for the two counts first (the entry sets them before it refuses a capacity of 0): the lists are as long as they need to be
            one = (C.c_int64 * 4)()
            rc = self.L.rtk_batch_fetch_seeds(self.h, i, C.byref(ns), one, C.byref(nw), one, 0)
            if rc != 0 and b"capacity" not in self.L.rtk_last_error():
                self.g._check(rc)
            cap = max(ns.value, nw.value)
        so, we = (C.c_int64 * (4 * max(1, cap)))(), (C.c_int64 * (4 * max(1, cap)))()
        self.g._check(self.L.rtk_batch_fetch_seeds(self.h, i, C.byref(ns), so, C.byref(nw), we, cap))
        f = lambda a, n: [(a[4 * j], a[4 * j + 1], a[4 * j + 2], a[4 * j + 3]) for j in range(n)]
        return f(so, ns.value), f(we, nw.value)

    def fetch(self):
        n = self.n
        os_, oq = (C.c_void_p * n)(), (C.c_void_p * n)()
        ol = (C.c_uint32 * n)()
        self.g._check(self.L.rtk_batch_fetch(self.h, os_, oq, ol))
        out = []
        for i in range(n):
            out.append((C.string_at(os_[i], ol[i]).decode(), C.string_at(oq[i], ol[i]).decode()))
            self.L.rtk_free(os_[i]); self.L.rtk_free(oq[i])
        return out

    def stats(self):
        s = RtkStats()
        self.g._check(self.L.rtk_batch_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    def close(self):
        if getattr(self, "h", None):
            self.L.rtk_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def myers_batch(queries, targets, ks=None, modes=None, want_path=False, use_iupac=True, lib_path=None, waves=0, lanes=False):
    """edlibAlign over a batch on the device: returns [(editDistance, endLocations, cigar)]. lanes=True: one problem per lane (stage entry
    rtk_myers_batch_lanes)."""
    L = load_library(lib_path)
    n = len(queries)
    bq = [_b(q) for q in queries]; bt = [_b(t) for t in targets]
    ks = ks if ks is not None else [-1] * n
    modes = modes if modes is not None else [0] * n
    qa = (C.c_char_p * n)(*bq); ta = (C.c_char_p * n)(*bt)
    ql = (C.c_uint32 * n)(*[len(x) for x in bq]); tl = (C.c_uint32 * n)(*[len(x) for x in bt])
    ka = (C.c_int32 * n)(*ks); ma = (C.c_int32 * n)(*modes)
    cap_locs = max(len(x) for x in bt) + 2 if n else 2
    cap_cig = 4 * (max((len(x) for x in bq), default=0) + max((len(x) for x in bt), default=0)) + 16
    dist = (C.c_int32 * n)(); nloc = (C.c_int32 * n)(); locs = (C.c_int32 * (n * cap_locs))()
    cig = C.create_string_buffer(n * cap_cig) if want_path else None
    if lanes:  # one problem per lane (stage entry; csrc/hip/rtk_myers_lane.h)
        rc = L.rtk_myers_batch_lanes(n, qa, ql, ta, tl, ka, ma, 1 if want_path else 0, 1 if use_iupac else 0, dist, nloc, locs, cap_locs, cig, cap_cig)
    elif waves > 1:  # the multi-wave schedule of the second pass's whole-read alignment (stage entry)
        rc = L.rtk_myers_batch_waves(n, qa, ql, ta, tl, ka, ma, 1 if want_path else 0, 1 if use_iupac else 0, dist, nloc, locs, cap_locs, cig, cap_cig, waves)
    else:
        rc = L.rtk_myers_batch(n, qa, ql, ta, tl, ka, ma, 1 if want_path else 0, 1 if use_iupac else 0, dist, nloc, locs, cap_locs, cig, cap_cig)
    if rc != 0:
        raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))
    out = []
    for i in range(n):
        el = [locs[i * cap_locs + j] for j in range(min(nloc[i], cap_locs))] if dist[i] >= 0 else []
        c = ""
        if want_path:
            c = cig.raw[i * cap_cig:(i + 1) * cap_cig].split(b"\0", 1)[0].decode()
        out.append((dist[i], el, c))
    return out


def _u64_array(a):
    """(owner, pointer, length) of a sequence of k-mers as uint64_t[]; a numpy array is passed without a copy when it already is one of uint64."""
    if hasattr(a, "ctypes"):
        import numpy as np
        arr = np.ascontiguousarray(a, dtype=np.uint64)
        return arr, arr.ctypes.data_as(C.POINTER(C.c_uint64)), int(arr.size)
    arr = (C.c_uint64 * max(1, len(a)))(*[int(x) for x in a])
    return arr, arr, len(a)


def rescue_reads(lr_kmers, sr_kmers, seqs, k=31, min_positions=31, device=0, stats=None, lib_path=None):
    """The unmapped-read rescue of `correct -u` (retrieveMissingReads, src/Graph.cpp:3857-4131; DESIGN.md section 4 [A11]) over rtk_rescue_begin / _chunk / _end:
    lr_kmers / sr_kmers = sorted canonical k-mers seen at least twice in the long reads / the mapped short reads; returns [bool] per read of seqs: at least
    min_positions start positions spell a k-mer of lr_kmers that is not in sr_kmers. stats (a dict) receives n_positions_probed and n_hits."""
    L = load_library(lib_path)
    if L.rtk_api_revision() < 9:
        raise RtkError("%s is of interface revision %d: the rescue entries came with revision 9" % (L._name, L.rtk_api_revision()))
    keep_lr, p_lr, n_lr = _u64_array(lr_kmers)
    keep_sr, p_sr, n_sr = _u64_array(sr_kmers)
    job = C.c_void_p()

    def check(rc):
        if rc != 0:
            raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))

    check(L.rtk_rescue_begin(device, k, p_lr, n_lr, p_sr, n_sr, min_positions, C.byref(job)))
    out = []
    try:
        bs = [_b(s) for s in seqs]
        i = 0
        while i < len(bs):  # chunks of at most 48 MB of characters and 2 M reads
            j, size = i, 0
            while j < len(bs) and (j == i or (size + len(bs[j]) + 1 <= (48 << 20) and j - i < (2 << 20))):
                size += len(bs[j]) + 1; j += 1
            starts, at = (C.c_uint64 * (j - i))(), 0
            for r in range(i, j):
                starts[r - i] = at; at += len(bs[r]) + 1
            chars = b"\n".join(bs[i:j]) + b"\n"
            keep = (C.c_ubyte * (j - i))()
            check(L.rtk_rescue_chunk(job, chars, len(chars), starts, j - i, keep))
            out.extend(bool(x) for x in keep)
            i = j
    except Exception:
        L.rtk_rescue_end(job, None, None)
        raise
    probed, hits = C.c_uint64(), C.c_uint64()
    check(L.rtk_rescue_end(job, C.byref(probed), C.byref(hits)))
    if stats is not None:
        stats["n_positions_probed"], stats["n_hits"] = probed.value, hits.value
    return out


QV_CHUNK_CHARS = 48 << 20  # characters per rtk_qv_chunk call of qv_reads, separators included (the entry takes 64 MB)


def qv_span(lib_path=None):
    """Start positions one wave of k_qv takes at a time (rtk_qv_span): tests place read lengths and piece sizes around it."""
    L = load_library(lib_path)
    if not hasattr(L, "rtk_qv_begin"):
        raise RtkError("%s has no rtk_qv entries" % L._name)
    return int(L.rtk_qv_span())


def qv_reads(solid_kmers, seqs, k=31, device=0, max_piece=None, lib_path=None, threads=1, stats=None):
    """The k-mer QV counts of rtk_qv (DESIGN.md section 4 [A17]) over rtk_qv_begin / _chunk / _end: solid_kmers = sorted distinct canonical k-mers (as
    rtk_index_count_kmers returns them); returns ([windows], [found]) per read of seqs: the start positions whose k characters are all A/C/G/T (either case) and
    those whose canonical k-mer is in the set. Chunks are laid out as rescue_reads lays them out; a read longer than max_piece characters (default: what a chunk
    holds) is cut into pieces that overlap by k - 1 characters and added up again, and a chunk holds max_piece + 1 characters at the most (tests lower it to get many
    chunks from little text). threads=2 feeds the chunks from two threads. stats (a dict) receives n_chunks, n_windows and n_found."""
    L = load_library(lib_path)
    if not hasattr(L, "rtk_qv_begin"):
        raise RtkError("%s has no rtk_qv entries" % L._name)
    if max_piece is None:
        max_piece = QV_CHUNK_CHARS - 1
    if max_piece < k or max_piece > QV_CHUNK_CHARS - 1:
        raise ValueError("max_piece must lie in k .. %d" % (QV_CHUNK_CHARS - 1))
    keep_solid, p_solid, n_solid = _u64_array(solid_kmers)
    bs = [_b(s) for s in seqs]
    pieces = []  # (read, piece text)
    for r, s in enumerate(bs):
        a = 0
        while True:
            pieces.append((r, s[a:a + max_piece]))
            if a + max_piece >= len(s):
                break
            a += max_piece - (k - 1)
    chunks, i = [], 0  # [i, j) of pieces: at most max_piece + 1 characters and 2 M pieces
    while i < len(pieces):
        j, size = i, 0
        while j < len(pieces) and size + len(pieces[j][1]) + 1 <= max_piece + 1 and j - i < (2 << 20):
            size += len(pieces[j][1]) + 1; j += 1
        chunks.append((i, j)); i = j
    job = C.c_void_p()

    def check(rc):
        if rc != 0:
            raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))

    check(L.rtk_qv_begin(device, k, p_solid, n_solid, C.byref(job)))
    windows, found = [0] * len(bs), [0] * len(bs)
    results = [None] * len(chunks)

    def run(c):
        i, j = chunks[c]
        starts, at = (C.c_uint64 * (j - i))(), 0
        for p in range(i, j):
            starts[p - i] = at; at += len(pieces[p][1]) + 1
        chars = b"\n".join(t for _, t in pieces[i:j]) + b"\n"
        w, f = (C.c_uint32 * (j - i))(), (C.c_uint32 * (j - i))()
        check(L.rtk_qv_chunk(job, chars, len(chars), starts, j - i, w, f))
        results[c] = (list(w), list(f))

    try:
        if threads <= 1:
            for c in range(len(chunks)):
                run(c)
        else:
            import threading
            errors = []

            def feed(t):
                try:
                    for c in range(t, len(chunks), threads):
                        run(c)
                except Exception as e:  # noqa: BLE001 (handed to the caller below)
                    errors.append(e)

            th = [threading.Thread(target=feed, args=(t,)) for t in range(threads)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            if errors:
                raise errors[0]
    except Exception:
        L.rtk_qv_end(job, None, None)
        raise
    n_windows, n_found = C.c_uint64(), C.c_uint64()
    check(L.rtk_qv_end(job, C.byref(n_windows), C.byref(n_found)))
    for c, (i, j) in enumerate(chunks):
        w, f = results[c]
        for p in range(i, j):
            windows[pieces[p][0]] += w[p - i]; found[pieces[p][0]] += f[p - i]
    if (sum(windows), sum(found)) != (n_windows.value, n_found.value):
        raise RtkError("rtk_qv: the pieces add up to %d windows / %d found, the device counted %d / %d" % (sum(windows), sum(found), n_windows.value, n_found.value))
    if stats is not None:
        stats["n_chunks"], stats["n_windows"], stats["n_found"] = len(chunks), n_windows.value, n_found.value
    return windows, found


def identity_reads(ref_records, reads, truth, device=0, lib_path=None, max_chunk=None, threads=1, max_len=None, stats=None):
    """The distances of rtk_identity (DESIGN.md section 4 [A19]) over rtk_identity_begin / _chunk / _end: ref_records = the records of the reference, reads = the
    read sequences, truth = per read (record number, 0-based start, length, reverse strand?). Returns per read the exact unit-cost NW edit distance to its
    stretch of the reference, reverse-complemented when the strand says so; reference and reads are upper-cased, bytes are equal iff identical. Chunks are laid
    out as qv_reads lays them out: whole reads, max_chunk characters with their separators (default: what qv_reads takes; tests lower it to get many chunks from
    little text; a chunk holds one read at the least). threads=2 feeds the chunks from two threads. max_len (default: the longest read or stretch) sizes the
    device's work areas. The returned sum is checked against the device's. stats (a dict) receives n_chunks, n_pairs and sum_dist."""
    L = load_library(lib_path)
    if not hasattr(L, "rtk_identity_begin"):
        raise RtkError("%s has no rtk_identity entries" % L._name)
    if len(reads) != len(truth):
        raise ValueError("one truth entry per read")
    if max_chunk is None:
        max_chunk = QV_CHUNK_CHARS
    recs = [_b(r).upper() for r in ref_records]
    bs = [_b(s).upper() for s in reads]
    offs = (C.c_uint64 * (len(recs) + 1))()
    for r, t in enumerate(recs):
        offs[r + 1] = offs[r] + len(t)
    text = b"".join(recs)
    if max_len is None:
        max_len = max([len(s) for s in bs] + [int(t[2]) for t in truth] + [1])
    chunks, i = [], 0  # [i, j) of reads
    while i < len(bs):
        j, size = i, 0
        while j < len(bs) and (j == i or size + len(bs[j]) + 1 <= max_chunk) and j - i < (2 << 20):
            size += len(bs[j]) + 1; j += 1
        chunks.append((i, j)); i = j
    job = C.c_void_p()

    def check(rc):
        if rc != 0:
            raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))

    check(L.rtk_identity_begin(device, text, len(text), offs, len(recs), max_len, C.byref(job)))
    out = [0] * len(bs)

    def run(c):
        i, j = chunks[c]
        n = j - i
        starts, rec, t_start, t_len, rev = (C.c_uint64 * n)(), (C.c_uint32 * n)(), (C.c_uint64 * n)(), (C.c_uint32 * n)(), (C.c_ubyte * n)()
        at = 0
        for p in range(i, j):
            starts[p - i] = at; at += len(bs[p]) + 1
            rec[p - i], t_start[p - i], t_len[p - i], rev[p - i] = int(truth[p][0]), int(truth[p][1]), int(truth[p][2]), 1 if truth[p][3] else 0
        chars = b"\n".join(bs[i:j]) + b"\n"
        d = (C.c_int32 * n)()
        check(L.rtk_identity_chunk(job, chars, len(chars), starts, n, rec, t_start, t_len, rev, d))
        out[i:j] = list(d)

    try:
        if threads <= 1:
            for c in range(len(chunks)):
                run(c)
        else:
            import threading
            errors = []

            def feed(t):
                try:
                    for c in range(t, len(chunks), threads):
                        run(c)
                except Exception as e:  # noqa: BLE001 (handed to the caller below)
                    errors.append(e)

            th = [threading.Thread(target=feed, args=(t,)) for t in range(threads)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            if errors:
                raise errors[0]
    except Exception:
        L.rtk_identity_end(job, None, None)
        raise
    n_pairs, sum_dist = C.c_uint64(), C.c_uint64()
    check(L.rtk_identity_end(job, C.byref(n_pairs), C.byref(sum_dist)))
    if (len(bs), sum(out)) != (n_pairs.value, sum_dist.value):
        raise RtkError("rtk_identity: the chunks add up to %d pairs / distance %d, the device counted %d / %d" % (len(bs), sum(out), n_pairs.value, sum_dist.value))
    if stats is not None:
        stats["n_chunks"], stats["n_pairs"], stats["sum_dist"] = len(chunks), n_pairs.value, sum_dist.value
    return out


MODE_SHW_BY_COLUMN, MODE_NW_PREFIX, MODE_NW_PREFIX_LAST, MODE_NW_PREFIX_LAST_COLUMN = 3, 4, 5, 6  # test-only modes of myers_batch (include/ratatosk_hip.h)


def myers_column_last_routes(lib_path=None):
    """(problems taken by the column route, problems answered by the calls it replaces) of this thread's last myers_batch call in modes 3 / 4 / 5."""
    L = load_library(lib_path)
    a, b = C.c_uint64(), C.c_uint64()
    L.rtk_myers_column_last_routes.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]; L.rtk_myers_column_last_routes.restype = None
    L.rtk_myers_column_last_routes(C.byref(a), C.byref(b))
    return a.value, b.value


def myers_lanes_last_routes(lib_path=None):
    """(problems computed one per lane, problems handed on to the wave route) of this thread's last myers_batch(..., lanes=True) call."""
    L = load_library(lib_path)
    a, b = C.c_uint64(), C.c_uint64()
    L.rtk_myers_lanes_last_routes.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]; L.rtk_myers_lanes_last_routes.restype = None
    L.rtk_myers_lanes_last_routes(C.byref(a), C.byref(b))
    return a.value, b.value


SETS_UNION, SETS_INTER, SETS_DIFF, SETS_INTER_COUNT, SETS_SORT_PAIRS, SETS_RADIX_U32, SETS_RADIX_PAIRS_U32, SETS_BM_LOWEST, SETS_BM8_LOWEST, SETS_RADIX_TAGGED, SETS_COLOUR_UNIVERSE = range(11)  # operations of sets_batch
SETS_OK, SETS_NOT_IN_BUILD, SETS_DECLINED = 0, 1, 2  # its per-problem statuses


def sets_batch(problems, lib_path=None):
    """The wave set primitives of the region stage on the device, one problem per wavefront in one launch (stage entry rtk_sets_batch, include/ratatosk_hip.h).
    problems: [(op, a, b, scalar)] with a and b sequences of 32-bit words (SETS_SORT_PAIRS: sequences of 64-bit keys and values). Returns [(words, result, status)]:
    the output words of the problem (SETS_SORT_PAIRS: (keys, values) as 64-bit integers), the operation's scalar result and SETS_OK or SETS_NOT_IN_BUILD."""
    import numpy as np
    L = load_library(lib_path)
    if L.rtk_api_revision() < 10:
        raise RtkError("%s is of interface revision %d: rtk_sets_batch came with revision 10" % (L._name, L.rtk_api_revision()))
    n = len(problems)
    keep, off = [], [0]
    ops = (C.c_uint32 * max(1, n))(); na = (C.c_uint32 * max(1, n))(); nb = (C.c_uint32 * max(1, n))(); sc = (C.c_uint32 * max(1, n))()
    pa = (C.POINTER(C.c_uint32) * max(1, n))(); pb = (C.POINTER(C.c_uint32) * max(1, n))()
    for i, (op, a, b, scalar) in enumerate(problems):
        if op == SETS_SORT_PAIRS:  # 64-bit words travel as (low, high) pairs of 32-bit words
            a = np.ascontiguousarray(a, dtype="<u8"); b = np.ascontiguousarray(b, dtype="<u8")
            count_a, count_b, a, b = int(a.size), int(b.size), a.view("<u4"), b.view("<u4")
        else:
            a = np.ascontiguousarray(a, dtype=np.uint32); b = np.ascontiguousarray(b, dtype=np.uint32)
            count_a, count_b = int(a.size), int(b.size)
        keep.append((a, b))
        ops[i], na[i], nb[i], sc[i] = op, count_a, count_b, scalar
        pa[i] = a.ctypes.data_as(C.POINTER(C.c_uint32)); pb[i] = b.ctypes.data_as(C.POINTER(C.c_uint32))
        need = {SETS_UNION: count_a + count_b, SETS_INTER: count_a, SETS_DIFF: count_a, SETS_INTER_COUNT: 0, SETS_SORT_PAIRS: 4 * count_a, SETS_RADIX_U32: count_a,
                SETS_RADIX_PAIRS_U32: 2 * count_a, SETS_BM_LOWEST: min(scalar, count_b), SETS_BM8_LOWEST: min(scalar, count_b),
                SETS_RADIX_TAGGED: 2 * count_a, SETS_COLOUR_UNIVERSE: 2 + count_a + 2 * count_b * max(1, (count_a + 63) // 64)}.get(op, 0)
        off.append(off[-1] + need)
    out = np.zeros(max(1, off[-1]), dtype=np.uint32)
    offs = (C.c_uint64 * (n + 1))(*off)
    out_n = (C.c_uint32 * max(1, n))(); res = (C.c_uint32 * max(1, n))(); st = (C.c_uint32 * max(1, n))()
    rc = L.rtk_sets_batch(n, ops, pa, na, pb, nb, sc, out.ctypes.data_as(C.POINTER(C.c_uint32)), offs, out_n, res, st)
    if rc != 0:
        raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))
    ret = []
    for i, (op, _, _, _) in enumerate(problems):
        if out_n[i] > off[i + 1] - off[i]:
            raise RtkError("rtk_sets_batch: problem %d reports %d output words for a slice of %d" % (i, out_n[i], off[i + 1] - off[i]))
        w = out[off[i]:off[i] + out_n[i]]
        if op == SETS_SORT_PAIRS and st[i] == SETS_OK:
            h = len(w) // 2
            words = (w[:h].copy().view("<u8").tolist(), w[h:].copy().view("<u8").tolist())
        else:
            words = w.tolist()
        ret.append((words, int(res[i]), int(st[i])))
    return ret


def index_subsample_events(events, n_unitigs, bin_of_unitig, forced_candidate, bin_is_sampled, mcv, rate, seed=1, device=0, lib_path=None):
    """The colour subsampling of the index build on the device (stage entry rtk_index_subsample_events, include/ratatosk_hip.h: the device function behind
    rtk_index_colour_end_subsampled; the rule: DESIGN.md section 4 [A12]). events: words unitig << 32 | id, ascending and distinct; bin_of_unitig[u] in 0 .. len(bin_is_sampled) - 1
    or 255; forced_candidate[u] and bin_is_sampled[j] 0 or 1. Returns (kept events with their ids renumbered, as a numpy array of uint64; distinct ids before; after)."""
    import numpy as np
    L = load_library(lib_path)
    missing = [s for s in ("rtk_index_colour_cov", "rtk_index_colour_end_subsampled", "rtk_index_subsample_events") if not hasattr(L, s)]
    if missing:
        raise RtkError("%s lacks %s (colour subsampling: appended at interface revision 10)" % (L._name, ", ".join(missing)))
    ev = np.ascontiguousarray(events, dtype=np.uint64)
    bins = np.ascontiguousarray(bin_of_unitig, dtype=np.uint8); forced = np.ascontiguousarray(forced_candidate, dtype=np.uint8); sampled = np.ascontiguousarray(bin_is_sampled, dtype=np.uint8)
    if bins.size != n_unitigs or forced.size != n_unitigs:
        raise RtkError("index_subsample_events: bin_of_unitig and forced_candidate hold one entry per unitig")
    out = np.zeros(max(1, ev.size), dtype=np.uint64)
    n_out, before, after = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    u8, u64 = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint64)
    rc = L.rtk_index_subsample_events(device, ev.ctypes.data_as(u64), ev.size, n_unitigs, bins.ctypes.data_as(u8), forced.ctypes.data_as(u8), sampled.ctypes.data_as(u8), sampled.size, mcv,
                                      float(rate), seed, out.ctypes.data_as(u64), C.byref(n_out), C.byref(before), C.byref(after))
    if rc != 0:
        raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))
    return out[:n_out.value].copy(), before.value, after.value


def index_merge_events(events, n_unitigs, device=0, lib_path=None):
    """The merging of the ids of read pairs that lie on the same unitigs, on the device (stage entry rtk_index_merge_events, include/ratatosk_hip.h: the device
    function behind rtk_index_colour_merge; the rule: DESIGN.md section 4 [A13]). events: words unitig << 32 | id, ascending and distinct, unitigs < n_unitigs.
    Returns (merged events with their new ids, ascending and distinct, as a numpy array of uint64; distinct ids before; after)."""
    import numpy as np
    L = load_library(lib_path)
    missing = [s for s in ("rtk_index_colour_merge", "rtk_index_colour_merge_classes", "rtk_index_merge_events") if not hasattr(L, s)]
    if missing:
        raise RtkError("%s lacks %s (merged ids: appended at interface revision 10)" % (L._name, ", ".join(missing)))
    ev = np.ascontiguousarray(events, dtype=np.uint64)
    out = np.zeros(max(1, ev.size), dtype=np.uint64)
    n_out, before, after = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    u64 = C.POINTER(C.c_uint64)
    rc = L.rtk_index_merge_events(device, ev.ctypes.data_as(u64), ev.size, n_unitigs, out.ctypes.data_as(u64), C.byref(n_out), C.byref(before), C.byref(after))
    if rc != 0:
        raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))
    return out[:n_out.value].copy(), before.value, after.value


def index_colour_reads(unitigs, k, reads, ids=None, quals=None, q_min=0, device=0, lib_path=None, chunks=None):
    """Colour events and k-mer coverage of `unitigs` under `reads`, on the device: one job over rtk_index_colour_begin, one rtk_index_colour_chunk or
    rtk_index_colour_chunk_q per chunk, rtk_index_colour_end (include/ratatosk_hip.h; the base-confidence rule: DESIGN.md section 4 [A14]). reads[r] colours with
    ids[r] (default: r). quals: None, or one entry per read -- its quality string, or None. A chunk whose reads all have a quality string goes through
    rtk_index_colour_chunk_q with q_min (a base whose quality byte is below q_min is no base), one whose reads have none through rtk_index_colour_chunk; a chunk
    that mixes the two is refused. chunks: the read indices at which a new chunk begins (default: one chunk). A library without rtk_index_colour_chunk_q raises an
    RtkError that names it as soon as a chunk needs it. Returns (events unitig << 32 | id, ascending and distinct; k-mers mapped per unitig) as numpy uint64 arrays."""
    import numpy as np
    L = load_library(lib_path)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.rtk_index_colour_begin.argtypes = [C.c_int, C.c_int, C.c_char_p, u64p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.rtk_index_colour_chunk.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, u64p, u32p, C.c_uint32]
    L.rtk_index_colour_end.argtypes = [C.c_void_p, C.POINTER(u64p), u64p, C.POINTER(u64p)]

    def as_bytes(x):
        return x if isinstance(x, bytes) else x.encode()

    reads = [as_bytes(r) for r in reads]
    ids = list(range(len(reads))) if ids is None else list(ids)
    quals = [None] * len(reads) if quals is None else [None if q is None else as_bytes(q) for q in quals]
    if len(ids) != len(reads) or len(quals) != len(reads):
        raise ValueError("index_colour_reads: ids and quals need one entry per read")
    for r, q in zip(reads, quals):
        if q is not None and len(q) != len(r):
            raise ValueError("index_colour_reads: a quality string is as long as its read")
    cuts = [0] + sorted(chunks or []) + [len(reads)]
    parts = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if a < b]
    for a, b in parts:
        n_q = sum(q is not None for q in quals[a:b])
        if n_q not in (0, b - a):
            raise ValueError("index_colour_reads: reads %d .. %d: a chunk holds reads with qualities or reads without, not both" % (a, b))
        if n_q and not hasattr(L, "rtk_index_colour_chunk_q"):
            raise RtkError("%s lacks rtk_index_colour_chunk_q (colouring by base confidence: appended at interface revision 10)" % L._name)

    def ok(rc):
        if rc != 0:
            raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))

    seqs = [as_bytes(u) for u in unitigs]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(u) for u in seqs], dtype=np.uint64)
    job = C.c_void_p()
    ok(L.rtk_index_colour_begin(device, k, b"".join(seqs), off.ctypes.data_as(u64p), len(seqs), C.byref(job)))
    try:
        for a, b in parts:
            chars = b"".join(r + b"\n" for r in reads[a:b])
            starts = np.zeros(b - a, dtype=np.uint64)
            starts[1:] = np.cumsum([len(r) + 1 for r in reads[a:b - 1]], dtype=np.uint64)
            cid = np.ascontiguousarray(ids[a:b], dtype=np.uint32)
            if quals[a] is None:
                ok(L.rtk_index_colour_chunk(job, chars, len(chars), starts.ctypes.data_as(u64p), cid.ctypes.data_as(u32p), b - a))
            else:
                qs = b"".join(q + b"\0" for q in quals[a:b])  # (the byte beside a separator is not looked at)
                ok(L.rtk_index_colour_chunk_q(job, chars, qs, q_min, len(chars), starts.ctypes.data_as(u64p), cid.ctypes.data_as(u32p), b - a))
    except BaseException:
        L.rtk_index_colour_end(job, None, None, None)
        raise
    ev_p, cov_p, n_ev = u64p(), u64p(), C.c_uint64(0)
    ok(L.rtk_index_colour_end(job, C.byref(ev_p), C.byref(n_ev), C.byref(cov_p)))
    try:
        events = np.ctypeslib.as_array(ev_p, shape=(max(1, n_ev.value),))[:n_ev.value].copy()
        cov = np.ctypeslib.as_array(cov_p, shape=(len(seqs),)).copy()
    finally:
        L.rtk_free(ev_p); L.rtk_free(cov_p)
    return events, cov


SNP_FIRST_PER_SITE = 1


def index_snp_candidates(unitigs, k, searched=None, first_per_site=False, device=0, lib_path=None):
    """The candidate search of the SNP annotations of an index build, on the device (stage entry rtk_index_snp_candidates, include/ratatosk_hip.h; the split between
    this search and the host's replay: DESIGN.md section 8). unitigs: sequences of A/C/G/T, each of at least k bases, no canonical k-mer twice; searched: None, or one
    flag per unitig -- the windows of a flagged unitig are queried, every unitig is found as a neighbour. Returns the list of (u, p, j, alt, w): window p of unitig u with
    base alt (A=0 .. T=3) at offset j is a k-mer of unitig w != u; ascending by (u, p, j, alt). first_per_site: of the candidates with equal (u, p + j, alt) only the
    one with the smallest p."""
    import numpy as np
    L = load_library(lib_path)
    if not hasattr(L, "rtk_index_snp_candidates"):
        raise RtkError("%s lacks rtk_index_snp_candidates (SNP candidates: appended at interface revision 10)" % L._name)
    seqs = [_b(u) for u in unitigs]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(u) for u in seqs], dtype=np.uint64)
    flags = None
    if searched is not None:
        flags = np.ascontiguousarray([1 if f else 0 for f in searched], dtype=np.uint8)
        if flags.size != len(seqs):
            raise ValueError("index_snp_candidates: searched holds one flag per unitig")
    u64p = C.POINTER(C.c_uint64)
    cand, n = u64p(), C.c_uint64(0)
    rc = L.rtk_index_snp_candidates(device, k, b"".join(seqs), off.ctypes.data_as(u64p), len(seqs), None if flags is None else flags.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                    SNP_FIRST_PER_SITE if first_per_site else 0, C.byref(cand), C.byref(n))
    if rc != 0:
        raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))
    try:
        w = np.ctypeslib.as_array(cand, shape=(max(1, 2 * n.value),))[:2 * n.value].copy() if n.value else np.zeros(0, dtype=np.uint64)
    finally:
        L.rtk_free(cand)
    w0, w1 = w[0::2], w[1::2]
    return list(zip((w0 >> np.uint64(32)).tolist(), (w0 & np.uint64(0xFFFFFFFF)).tolist(), (w1 >> np.uint64(40)).tolist(), ((w1 >> np.uint64(32)) & np.uint64(3)).tolist(), (w1 & np.uint64(0xFFFFFFFF)).tolist()))


def index_snp_plan(unitigs, k, searched=None, room=0, device=0, lib_path=None):
    """What index_snp_candidates would do for these unitigs with `room` bytes of device memory (0: what the stage itself would go by now -- the free memory, or
    RTK_INDEX_SNP_MEM when that is lower), worked out by the stage's own code without allocating anything (rtk_index_snp_plan, include/ratatosk_hip.h). Only the lengths
    of the unitigs count. Returns (passes, need_one_pass, need_min): the number of passes over partitions of the key space (0: nothing fits; RTK_INDEX_SNP_PASSES forces
    it), the bytes of the single pass, the bytes of the smallest plan."""
    import numpy as np
    L = load_library(lib_path)
    if not hasattr(L, "rtk_index_snp_plan"):
        raise RtkError("%s lacks rtk_index_snp_plan (SNP candidates in passes: appended at interface revision 10)" % L._name)
    off = np.zeros(len(unitigs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(u) for u in unitigs], dtype=np.uint64)
    flags = None
    if searched is not None:
        flags = np.ascontiguousarray([1 if f else 0 for f in searched], dtype=np.uint8)
        if flags.size != len(unitigs):
            raise ValueError("index_snp_plan: searched holds one flag per unitig")
    passes, one, least = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    rc = L.rtk_index_snp_plan(device, k, off.ctypes.data_as(C.POINTER(C.c_uint64)), len(unitigs), None if flags is None else flags.ctypes.data_as(C.POINTER(C.c_ubyte)), room,
                              C.byref(passes), C.byref(one), C.byref(least))
    if rc != 0:
        raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))
    return passes.value, one.value, least.value


def name_hash(name):
    """The hash of a read name for --pair-by-name (DESIGN.md section 4 [A18]; csrc/common/name_hash.hpp): 64-bit FNV-1a over the bytes of the name (what the readers
    hand over: the header up to the first blank, without a trailing /1 or /2), then the mixer of the k-mer tables. Pure Python."""
    m, h = (1 << 64) - 1, 0xcbf29ce484222325
    for c in _b(name):
        h = ((h ^ c) * 0x100000001b3) & m
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & m
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & m
    return h ^ (h >> 33)


def index_pair_ids(hashes, device=0, lib_path=None):
    """The colour ids of the read pairs by name, on the device (stage entry rtk_index_pair_ids, include/ratatosk_hip.h): hashes[r] = the name hash of record r of the
    colouring input, in input order. Returns (ids, n_ids): ids[r] = the number of distinct hashes first seen before the first record of hashes[r] (a list), and the
    number of distinct hashes. RTK_INDEX_PAIR_PASSES / RTK_INDEX_PAIR_MEM are read at the call."""
    import numpy as np
    L = load_library(lib_path)
    if not hasattr(L, "rtk_index_pair_ids"):
        raise RtkError("%s lacks rtk_index_pair_ids (read pairs by name: appended at interface revision 10)" % L._name)
    h = np.ascontiguousarray(hashes, dtype=np.uint64)
    ids = np.zeros(max(1, h.size), dtype=np.uint32)
    n_ids = C.c_uint64(0)
    rc = L.rtk_index_pair_ids(device, h.ctypes.data_as(C.POINTER(C.c_uint64)) if h.size else None, h.size, ids.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n_ids))
    if rc != 0:
        raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))
    return ids[:h.size].tolist(), n_ids.value


def index_pair_plan(n, room=0, device=0, lib_path=None):
    """What index_pair_ids would do for n records with `room` bytes of device memory (0: what the stage itself would go by now -- the free memory, or
    RTK_INDEX_PAIR_MEM when that is lower), worked out by the stage's own code without allocating anything (rtk_index_pair_plan). Returns (passes, need_one_pass,
    need_min): the number of passes over equal ranges of the hash space (0: nothing fits; RTK_INDEX_PAIR_PASSES forces it), the bytes of the single pass, the bytes
    of the smallest plan."""
    L = load_library(lib_path)
    if not hasattr(L, "rtk_index_pair_plan"):
        raise RtkError("%s lacks rtk_index_pair_plan (read pairs by name: appended at interface revision 10)" % L._name)
    passes, one, least = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    rc = L.rtk_index_pair_plan(device, n, room, C.byref(passes), C.byref(one), C.byref(least))
    if rc != 0:
        raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))
    return passes.value, one.value, least.value


def index_cover_layout(sequences, k, chunks=None):
    """The chunks index_cover_crossings hands to the device for `sequences`, as (chars, starts, seq_numbers, first_positions) each: what rtk_index_cover_chunk
    takes. A sequence shorter than k + 1 characters holds no pair of windows and is left out (the numbers of the others stay those of the list). chunks: None
    (every sequence whole, all in one chunk), or the largest number of characters of a chunk, separators included: the sequences are then packed into chunks of
    that size in their order, and a sequence longer than a chunk is cut into pieces that overlap by k characters, so that every k + 1 consecutive characters lie
    whole inside exactly one piece. Character starts[r] + j of a chunk is position first_positions[r] + j of sequence seq_numbers[r]."""
    import numpy as np
    if chunks is not None and chunks < k + 3:
        raise ValueError("index_cover_crossings: a chunk holds at least k + 2 characters and a separator")
    pieces = []  # (sequence number, first position, characters)
    for n, s in enumerate(_b(x) for x in sequences):
        if len(s) < k + 1:
            continue
        a, room = 0, len(s) if chunks is None else chunks - 1
        while True:
            e = min(len(s), a + room)
            pieces.append((n, a, s[a:e]))
            if e == len(s):
                break
            a = e - k
    parts, cur, size = [], [], 0
    for pc in pieces:
        if cur and chunks is not None and size + len(pc[2]) + 1 > chunks:
            parts.append(cur); cur, size = [], 0
        cur.append(pc); size += len(pc[2]) + 1
    if cur:
        parts.append(cur)
    out = []
    for part in parts:
        starts = np.zeros(len(part), dtype=np.uint64)
        starts[1:] = np.cumsum([len(c) + 1 for _, _, c in part[:-1]], dtype=np.uint64)
        out.append((b"".join(c + b"\n" for _, _, c in part), starts, np.ascontiguousarray([n for n, _, _ in part], dtype=np.uint32),
                    np.ascontiguousarray([a for _, a, _ in part], dtype=np.uint64)))
    return out


def index_cover_crossings(unitigs, k, low_bits, sequences, device=0, lib_path=None, chunks=None):
    """Where `sequences` cross the recorded low-coverage edges of `unitigs`, on the device: one job over rtk_index_cover_begin, one rtk_index_cover_chunk per
    chunk, rtk_index_cover_end (include/ratatosk_hip.h; the rule: DESIGN.md section 4 [A16]). low_bits: one byte per unitig -- bit 1, 2, 4, 8 for the successor of
    the forward strand that appends A, C, G, T, the same << 4 for the reverse strand. chunks: how the sequences are cut and packed (index_cover_layout). Returns the
    list of (sequence number, p, u, v, direction, base), ascending by (sequence number, p): the bits are only read, nothing is cleared."""
    import numpy as np
    L = load_library(lib_path)
    if not hasattr(L, "rtk_index_cover_begin"):
        raise RtkError("%s lacks rtk_index_cover_begin / _chunk / _end (low-coverage edges covered: appended at interface revision 10)" % L._name)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    seqs = [_b(u) for u in unitigs]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(u) for u in seqs], dtype=np.uint64)
    low = np.ascontiguousarray(low_bits, dtype=np.uint8)
    if low.size != len(seqs):
        raise ValueError("index_cover_crossings: low_bits holds one byte per unitig")
    parts = index_cover_layout(sequences, k, chunks)

    def ok(rc):
        if rc != 0:
            raise RtkError("rtk error %d: %s" % (rc, L.rtk_last_error().decode()))

    job = C.c_void_p()
    ok(L.rtk_index_cover_begin(device, k, b"".join(seqs), off.ctypes.data_as(u64p), len(seqs), low.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(job)))
    try:
        for chars, starts, numbers, first in parts:
            ok(L.rtk_index_cover_chunk(job, chars, len(chars), starts.ctypes.data_as(u64p), numbers.ctypes.data_as(u32p), first.ctypes.data_as(u64p), len(numbers)))
    except BaseException:
        L.rtk_index_cover_end(job, None, None)
        raise
    out, n = u64p(), C.c_uint64(0)
    ok(L.rtk_index_cover_end(job, C.byref(out), C.byref(n)))
    try:
        w = np.ctypeslib.as_array(out, shape=(max(1, 2 * n.value),))[:2 * n.value].copy() if n.value else np.zeros(0, dtype=np.uint64)
    finally:
        L.rtk_free(out)
    w0, w1 = w[0::2], w[1::2]
    one = np.uint64(1)
    return list(zip((w0 >> np.uint64(32)).tolist(), (w0 & np.uint64(0xFFFFFFFF)).tolist(), (w1 >> np.uint64(33)).tolist(), ((w1 >> np.uint64(3)) & np.uint64(0x3FFFFFFF)).tolist(),
                    ((w1 >> np.uint64(2)) & one).tolist(), (w1 & np.uint64(3)).tolist()))


def run_pipelined(batches, opts=None):
    """Runs the batches in order with the seed stage of batch i+1 overlapping the region stage of batch i (two host threads,
    one HIP stream per batch). Results are the same as calling run() on each batch."""
    import threading
    prev, err = None, []

    def seeds(b):
        try:
            b.run_seeds(opts)
        except Exception as e:  # surfaced on the calling thread
            err.append(e)

    for b in batches:
        t = threading.Thread(target=seeds, args=(b,))
        t.start()
        if prev is not None:
            prev.run_regions(opts)
        t.join()
        if err:
            raise err[0]
        prev = b
    if prev is not None:
        prev.run_regions(opts)
