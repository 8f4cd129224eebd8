// Geometry of the Ukkonen band of a pass (host and device; tests/test_myers_band.py restates it).
#ifndef RTK_MYERS_BAND_H
#define RTK_MYERS_BAND_H
#include "rtk_wave.h"

// ---- band of a pass: diagonals dlo <= j - i <= dhi (i = query row, j = target column, 0-based) -----------------------------------------------
#define RTK_BAND_FULL (1 << 29)
#define RTK_BAND_INF 0x3fffffff      // score of a row outside the band
#define RTK_RING_MAX_BAND 4000       // widest band (diagonals) of the ring schedule: a lane must be done with word w before word w + 64 starts
struct RtkBand { int dlo, dhi; };
RTK_HD RtkBand rtk_band_full() { RtkBand b; b.dlo = -RTK_BAND_FULL; b.dhi = RTK_BAND_FULL; return b; }
// Ukkonen band of an NW problem of m rows and n columns whose distance is <= k (k is raised to |n - m| if smaller)
RTK_HD RtkBand rtk_band_nw(int m, int n, int k) {
    const int d = n - m, ad = d < 0 ? -d : d;
    const int h = k > ad ? (k - ad) / 2 : 0;
    RtkBand b; b.dlo = (d < 0 ? d : 0) - h; b.dhi = (d > 0 ? d : 0) + h; return b;
}
RTK_HD bool rtk_band_is_full(const RtkBand& b, int m, int n) { return b.dlo <= -m && b.dhi >= n; }
// words computed together share their column range: gran = 1 (ring: every word its own) or 64 (row blocks)
RTK_HD int rtk_band_clo(int w, int dlo, int gran) { const long long c = 64LL * ((w / gran) * gran) + dlo; return c < 0 ? 0 : static_cast<int>(c); }
RTK_HD int rtk_band_chi(int w, int W, int n, int dhi, int gran) { int wl = (w / gran) * gran + gran - 1; if (wl > W - 1) wl = W - 1; const long long c = 64LL * wl + 63 + dhi; return c > n - 1 ? n - 1 : static_cast<int>(c); }
// words that have a column at all: the band reaches row n - 1 - dlo at most
RTK_HD int rtk_band_words(int m, int n, int dlo) { const int W = (m + 63) >> 6; const long long r = static_cast<long long>(n) - 1 - dlo; if (r < 0) return 0; const long long w = (r >> 6) + 1; return w < W ? static_cast<int>(w) : W; }
// schedule of a banded pass: the ring (every word its own column range) when it pays and fits, row blocks otherwise
RTK_HD int rtk_band_gran(int m, int dlo, int dhi) { return (((m + 63) >> 6) > 64 && (dhi - dlo) <= RTK_RING_MAX_BAND) ? 1 : 64; }
// first guess of the distance of an NW problem (the top of a Hirschberg recursion): generous where the ring makes the width free
RTK_HD int rtk_band_guess(int m, int n) {
    const int d = n - m, ad = d < 0 ? -d : d, mn = m < n ? m : n;
    int g = ad + (mn / 8 > 64 ? mn / 8 : 64);
    if (g < RTK_RING_MAX_BAND - 100) g = RTK_RING_MAX_BAND - 100;
    return g < m + n ? g : m + n;
}
#endif
