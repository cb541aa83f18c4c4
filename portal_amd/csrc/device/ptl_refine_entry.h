// ptl_refine_entry.h -- the list-driven render entry of ONE frame: ptl_refine_walk (device/ptl_refine_common.h, spliced in front of this
// text) over the `*count` entries of `list`, each pixel shaded with the same glsl::shade_pixel as the render entry.  Both pieces go into
// the device half of ptl_entry.h for sources generated with flag bit 28 (PTL_FLAG_REFINE, codegen.cpp `apply_refine_entry`).
#if !defined(PTL_TELEPORT_MODULE)
extern "C" __global__ void PTL_LAUNCH_BOUNDS
ptl_render_refine_kernel(const unsigned int* __restrict__ list,   // refined pixels, y * width + x each
                         const unsigned int* __restrict__ count,  // how many of them
                         unsigned int* __restrict__ out_rgba8,    // the full frame pass 1 wrote, or null
                         float* __restrict__ out_rgba32f,         // same, 4 floats per pixel, or null
                         int width, int height,                    // full frame size
                         unsigned long long* __restrict__ segment_counter) {
    // (*count is workgroup-uniform: a scalar load)
    ptl_refine_walk(list, *count, out_rgba8, out_rgba32f, width, height, segment_counter, [](glsl::vec2 position) { return glsl::shade_pixel(position); });
}
#endif  // !PTL_TELEPORT_MODULE

