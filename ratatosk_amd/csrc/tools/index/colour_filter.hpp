// rtk_build_index --colour-reads with --colour-min-conf / --colour-max-qual / --colour-min-len: which bases and which reads colour a second-pass index (restates the
// part of addCoverage that runs with long_read_correct == true, src/Ratatosk.cpp:1228: the graph of the second pass is coloured by the reads of the first; DESIGN.md
// section 4 [A14]). One rule for the host routes here and for the device route (csrc/hip/rtk_index_colour.h rtk_index_colour_chunk_q, k_col_mask), which give the same bytes:
//   c_min  = (unsigned char)(min(M, 1.0) * (Q - 1) + 34.0): getQual(min_confidence_2nd_pass, out_qual = 1, max_qual) (src/Common.hpp:410-418, called at
//            src/Graph.cpp:1573) with its double-to-char truncation. Q = 40: M = 0 gives 34 ('"'), M = 0.5 gives 53 ('5'), M = 1 gives 73 ('I').
//   A base of a colouring read whose quality byte is below c_min (bytes compare unsigned) is no base (src/Graph.cpp:1806-1814, 1872-1880 write 'N' over it before the
//   k-mers are looked up): every k-mer window that holds it gives no event and no coverage. With M = 0 these are the '!' bases, which the first pass writes over the
//   stretches it could not anchor (src/Correction.cpp:170, 184).
//   A colouring read shorter than --colour-min-len (min_len_2nd_pass, -C; src/Graph.cpp:1796, 1870) gives no events and no coverage.
//   Helper reads given as a further --colour-reads fall under the rule as the reference's -a reads do (they sit in the same filename_seq_in); the -s reads never do.
// Deviations. (1) Opt-in: the reference applies -M 0.0 -C 3000 to every second-pass index; here nothing is filtered unless an option is given. (2) A read's id stays the
// number of colouring reads before it whether or not it, or a read before it, is left out (the reference numbers what it keeps): the routes number before they filter,
// and an index built from a copy of the file with the masked bases spelled 'N' is the same index. (3) With --colour-min-conf a colouring record without a quality string
// of its own length is an error that names the file (the reference would read through a null pointer); --colour-min-len alone takes FASTA.
#ifndef RTK_TOOLS_INDEX_COLOUR_FILTER_HPP
#define RTK_TOOLS_INDEX_COLOUR_FILTER_HPP

#include <cstddef>
#include <cstdint>

namespace rtk {

inline unsigned char colour_q_min(double min_conf, int max_qual) { return static_cast<unsigned char>((min_conf < 1.0 ? min_conf : 1.0) * static_cast<double>(max_qual - 1) + 34.0); }

// out[0 .. len) = seq with 'N' where the quality byte is below q_min
inline void colour_mask_bases(const char* seq, const char* qual, size_t len, unsigned char q_min, char* out) {
    for (size_t i = 0; i < len; ++i) out[i] = static_cast<unsigned char>(qual[i]) < q_min ? 'N' : seq[i];
}

} // namespace rtk

#endif
