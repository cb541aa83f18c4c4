// ptl_refine_slices_entry.h -- the list-driven render entry over the slices of ONE launch: ptl_refine_walk (device/ptl_refine_common.h,
// spliced in front of this text) once per slice.  Both pieces go into the device half of ptl_entry.h, behind the slices entry, for sources
// generated with flag bit 29 (PTL_FLAG_REFINE_SLICES, codegen.cpp `apply_refine_entry`).
//
// Slice z = blockIdx.z has its own list (`lists + z * list_stride`, `counts[z]` entries -- written by kernels/aa_edges_slices.hip), its
// own uniform block (`ptl_slices + z`, the buffer of blocks the slices render entry reads) and its own frame (`out_* + z *
// ptl_slice_pixels` pixels).  One list per slice, not one merged list with the slice packed into the entry: every lane of a workgroup then
// shades with the same block, its address is workgroup-uniform, and the uniform reads stay scalar loads -- what the slices entry is built
// around.
#if !defined(PTL_TELEPORT_MODULE)
extern "C" __global__ void PTL_LAUNCH_BOUNDS
ptl_render_refine_slices_kernel(const glsl::ptl_uniform_block* __restrict__ ptl_slices,  // the launch's buffer of uniform blocks
                                unsigned long long ptl_slice_pixels,                      // distance between two slices' frames, in pixels
                                const unsigned int* __restrict__ lists,                   // slice z: lists + z * list_stride, y * width + x each
                                unsigned long long list_stride,                           // distance between two lists, in entries
                                const unsigned int* __restrict__ counts,                  // counts[z]: entries of slice z
                                unsigned int* __restrict__ out_rgba8,                     // the frames pass 1 wrote, or null
                                float* __restrict__ out_rgba32f,                          // same, 4 floats per pixel, or null
                                int width, int height,                                     // full frame size (every slice's)
                                unsigned long long* __restrict__ segment_counter) {
    const unsigned int z = blockIdx.z;                                         // workgroup-uniform, like everything derived from it
    const glsl::ptl_uniform_block* const ptl_slice_block = ptl_slices + z;     // this slice's uniforms ...
    const unsigned int* const list = lists + (unsigned long long)z * list_stride;  // ... its list ...
    if (out_rgba8 != nullptr) out_rgba8 += (unsigned long long)z * ptl_slice_pixels;  // ... and its frame
    if (out_rgba32f != nullptr) out_rgba32f += 4ull * z * ptl_slice_pixels;
    const unsigned long long listed = counts[z];  // a scalar load; never read past the slice's own list, whatever the word holds
    const unsigned int n = (unsigned int)(listed < list_stride ? listed : list_stride);
    ptl_refine_walk(list, n, out_rgba8, out_rgba32f, width, height, segment_counter,
                    [ptl_slice_block](glsl::vec2 position) { return glsl::shade_pixel_in(position, ptl_slice_block); });
}
#endif  // !PTL_TELEPORT_MODULE

