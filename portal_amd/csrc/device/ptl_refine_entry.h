// ptl_refine_entry.h -- adaptive anti-aliasing, pass 3 of 3: the listed pixels again, with the frame's full `_aa_count`.
// Spliced into the device half of ptl_entry.h by the generator for sources generated with flag bit 28 (PTL_FLAG_REFINE,
// codegen.cpp `apply_refine_entry`); a source generated without the flag has no trace of it.
//
// `list` holds the pixel indices y * width + x that the classification kernel (kernels/aa_edges.hip) flagged, `*count` how many:
// both live in device memory and are read HERE, so the host never looks at them and nothing synchronises between the passes.
// The grid has a fixed size chosen from the frame size; workgroup b takes entries [256 c, 256 c + 256) for c = b, b + gridDim.x, ...
// until the count is reached -- a static stride, not a work queue.  A wave takes 64 consecutive entries, which the classification
// kernel produced together (8x8 tile after 8x8 tile of one 64x32 region): still a compact bundle of rays.  Each lane shades its
// own pixel with the same glsl::shade_pixel as the render entry -- a pixel's value does not depend on which lanes share its wave --
// and stores its own 4 bytes (and its own float4): no LDS transpose, the lanes of a wave are not a rectangle.
#if !defined(PTL_TELEPORT_MODULE)
extern "C" __global__ void PTL_LAUNCH_BOUNDS
ptl_render_refine_kernel(const unsigned int* __restrict__ list,   // refined pixels, y * width + x each
                         const unsigned int* __restrict__ count,  // how many of them
                         unsigned int* __restrict__ out_rgba8,    // the full frame pass 1 wrote, or null
                         float* __restrict__ out_rgba32f,         // same, 4 floats per pixel, or null
                         int width, int height,                    // full frame size
                         unsigned long long* __restrict__ segment_counter) {
    const int t = (int)threadIdx.x;
#ifdef PTL_COUNT_SEGMENTS
    const int lane = t & 63;
    ptl_segments_lds[t] = 0u;
#endif
#if defined(PTL_MATERIAL_TABLE) && PTL_MATERIAL_TABLE == 1
    {  // stage the Simple materials' constants in LDS once per workgroup, as the render entry does
        for (int k = (int)threadIdx.x; k < PTL_MATERIAL_TABLE_WORDS; k += (int)blockDim.x) glsl::ptl_material_table[k] = glsl::ptl_material_table_init[k];
        __syncthreads();
    }
#endif
#ifdef PTL_UNIFORMS_IN_LDS
    {  // stage the scene constants (portal matrices, uniforms) in LDS once per workgroup
        const unsigned int* src = reinterpret_cast<const unsigned int*>(&glsl::ptl_u);
        unsigned int* dst = reinterpret_cast<unsigned int*>(&glsl::ptl_lds_u);
        for (int i = t; i < (int)(sizeof(glsl::ptl_uniform_block) / 4); i += 256) dst[i] = src[i];
        __syncthreads();
    }
#endif
    const unsigned int n = *count;  // workgroup-uniform: a scalar load
    const unsigned int pixels = (unsigned int)width * (unsigned int)height;
    for (unsigned int first = blockIdx.x * 256u; first < n; first += gridDim.x * 256u) {
        const unsigned int i = first + (unsigned int)t;
        if (i >= n) continue;
        const unsigned int idx = list[i];
        if (idx >= pixels) continue;  // (never for a list the classification kernel wrote: a caller's own list stays inside the frame)
        const unsigned int py = idx / (unsigned int)width, px = idx - py * (unsigned int)width;
        const glsl::vec4 c = glsl::shade_pixel(glsl::vec2((float)px + 0.5f, (float)py + 0.5f));
        if (out_rgba32f != nullptr) *reinterpret_cast<float4*>(out_rgba32f + 4ul * idx) = make_float4(c.x, c.y, c.z, c.w);
        if (out_rgba8 != nullptr) out_rgba8[idx] = glsl::pack_rgba8(c);
    }
#ifdef PTL_COUNT_SEGMENTS
    if (segment_counter != nullptr) {
        unsigned int trips = ptl_segments_lds[t];
        for (int off = 32; off > 0; off >>= 1) trips += __shfl_down(trips, off, 64);
        if (lane == 0) atomicAdd(segment_counter, (unsigned long long)trips);
    }
#endif
}
#endif  // !PTL_TELEPORT_MODULE

