// Dump of a segment launch's geometry from the kernel's own functions (vd_segplan.h seg_table; vd_kernel_tg.h
// seg_bound, seg_nruns, seg_run, set up as vd_decode_tg sets up its SegWG): for every workgroup its first chunk,
// chunk count and five boundaries, then every run of its four segments.  tests/test_seg_predict.py compares the
// text line for line with the Python restatement in tests/seg_predict.py (dump_lines).  An absent table prints
// nothing.  Built with hipcc on the host; usage: seg_runs_dump nsimd mode packNum outputBits
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vd_kernel_tg.h"
#include "vd_segplan.h"

using namespace vd;

int main(int argc, char** argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: %s nsimd mode packNum outputBits\n", argv[0]);
        return 2;
    }
    const int nsimd = atoi(argv[1]), mode = atoi(argv[2]), ob = atoi(argv[4]);
    Geom geo{};
    geo.packNum = strtoull(argv[3], nullptr, 10);
    geo.nchunks = kChunks;
    if (mode < 0 || mode > 2 || (ob != 16 && ob != 32)) return 2;
    auto words32 = [&](uint32_t c) {  // (the kernel's lambda of the same name)
        const uint32_t w = chunk_range(geo, c).words;
        return ob == 32 ? w : (w + 1) / 2;
    };
    const std::vector<uint32_t> t = seg_table(nsimd, mode);
    for (size_t g = 0; g + 1 < t.size(); g++) {
        SegWG sw;
        sw.c0 = t[g];
        sw.k = (int)(t[g + 1] - sw.c0);
        sw.warm = Geom{}.segWarm;
        sw.W0 = words32(sw.c0);
        sw.W1 = sw.k > 1 ? words32(sw.c0 + 1) : 0u;
        sw.W2 = sw.k > 2 ? words32(sw.c0 + 2) : 0u;
        sw.W3 = sw.k > 3 ? words32(sw.c0 + 3) : 0u;
        printf("wg %zu c0 %u k %d bounds", g, sw.c0, sw.k);
        for (int q = 0; q <= kWaves; q++) {
            const SegPos b = seg_bound(sw, q);
            printf(" %d:%u", b.i, b.a);
        }
        printf("\n");
        for (int q = 0; q < kWaves; q++) {
            const SegPos b0 = seg_bound(sw, q), b1 = seg_bound(sw, q + 1);
            for (int r = 0; r < seg_nruns(b0, b1); r++) {
                const RunGeo rg = seg_run(sw, b0, b1, r);
                printf("run %zu %d %d %d %u %u %u %d %d\n", g, q, r, rg.i, rg.s0, rg.words, rg.E, rg.Xspec, rg.Xcmp);
            }
        }
    }
    return 0;
}
