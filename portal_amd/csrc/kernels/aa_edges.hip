// aa_edges.hip -- adaptive anti-aliasing, pass 2 of 3: which pixels of the one-sample frame sit on an edge?
//
// Contract (include/portal_amd.h; tests/adaptive_reference.py restates it in numpy).  P is an RGBA8 frame, T an
// integer in -1 .. 255.  Integers only:
//   d(x, y)      = max over dx, dy in {-1, 0, 1}, c in {R, G, B} of | P(clamp(x+dx), clamp(y+dy)).c - P(x, y).c |
//   refine(x, y) = d(x, y) > T                   coordinates clamp to the frame, alpha is ignored
// Output: the pixel indices y * W + x of the refined pixels as a dense uint32 list in device memory, and their number.
// T = -1 lists every pixel, T = 255 none.  The order of the list is free, but entries that are produced together are spatial
// neighbours: a workgroup appends its region as one run, 8x8 tile after 8x8 tile, so 64 consecutive entries are (pieces of) a few
// neighbouring tiles and the refine pass still traces compact bundles of rays.
//
// gfx950 mapping: a 256-thread workgroup owns a 64x32 pixel region (2 048 pixels; a 4K frame is 4 050 regions).
//   1. the region and its one-pixel halo, coordinates clamped, go into LDS once: 66 x 34 words (rows padded to 72), ~1.1 loads per pixel, so HBM
//      sees the frame once (4 B per pixel) plus the list;
//   2. each wave classifies eight 8x8 tiles (wave w: tile row w of the region), nine LDS reads per pixel, and keeps its eight
//      verdicts in a bit mask -- nothing is indexed dynamically, no scratch;
//   3. slots: ballot + popcount per tile inside the wave, an LDS prefix across the four waves, and ONE returning device-scope
//      add per workgroup on the count (a returning add on one word saturates near 88 per microsecond: one per wave would be
//      1.5 ms at 4K, one per region is ~46 us spread over the launch, and a region without edges issues none);
//   4. each lane stores its entries at base + tiles before + mbcnt.
#include "aa_edges_common.h"

extern "C" __global__ void __launch_bounds__(256)
ptl_aa_edges_kernel(const unsigned int* __restrict__ frame,  // P: width * height packed RGBA8 pixels
                    int width, int height, int threshold,
                    unsigned int* __restrict__ list,         // capacity width * height entries: cannot overflow
                    unsigned int* __restrict__ count) {      // zeroed on the stream before the launch (ptl_aa_edges)
    ptl_aa_edges_region(frame, width, height, threshold, list, count);
}
