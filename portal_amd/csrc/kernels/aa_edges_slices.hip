// aa_edges_slices.hip -- adaptive anti-aliasing of a batch of slices, pass 2 of 3: the classification of aa_edges.hip over a stack of
// one-sample frames in ONE launch.  Grid (ceil(W / 64), ceil(H / 32), n): slice z = blockIdx.z reads the frame at frames + z * slice_pixels,
// appends to its own list at lists + z * list_stride and counts in counts[z] -- the rule is applied to each slice on its own (a frame's
// border clamps to that frame, never to its neighbour in the stack), and a workgroup still reserves its slots with one returning add.
// One list per slice: the refine pass (device/ptl_refine_slices_entry.h) walks each with that slice's uniform block.
#include "aa_edges_common.h"

extern "C" __global__ void __launch_bounds__(256)
ptl_aa_edges_slices_kernel(const unsigned int* __restrict__ frames,  // slice z: width * height packed RGBA8 pixels at frames + z * slice_pixels
                           unsigned long long slice_pixels,
                           int width, int height, int threshold,
                           unsigned int* __restrict__ lists,          // slice z: capacity list_stride >= width * height entries, cannot overflow
                           unsigned long long list_stride,
                           unsigned int* __restrict__ counts) {       // counts[0 .. n) zeroed on the stream before the launch (ptl_aa_edges_slices)
    const unsigned long long z = blockIdx.z;
    ptl_aa_edges_region(frames + z * slice_pixels, width, height, threshold, lists + z * list_stride, counts + z);
}
