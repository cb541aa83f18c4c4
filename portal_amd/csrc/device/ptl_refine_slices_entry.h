// ptl_refine_slices_entry.h -- adaptive anti-aliasing of a batch of slices, pass 3 of 3: the listed pixels of every slice again, with
// that slice's full `_aa_count`.  Spliced into the device half of ptl_entry.h, behind the slices entry, for sources generated with flag
// bit 29 (PTL_FLAG_REFINE_SLICES, codegen.cpp `apply_refine_slices_entry`); a source generated without the flag has no trace of it.
//
// The refine entry of device/ptl_refine_entry.h over the slices of ONE launch: slice z = blockIdx.z has its own list
// (`lists + z * list_stride`, `counts[z]` entries -- written by kernels/aa_edges_slices.hip, read HERE), its own uniform block
// (`ptl_slices + z`, the buffer of blocks the slices render entry reads) and its own frame (`out_* + z * ptl_slice_pixels` pixels).
// One list per slice, not one merged list with the slice packed into the entry: every lane of a workgroup then shades with the same
// block, its address is workgroup-uniform, and the uniform reads stay scalar loads -- what the slices entry is built around.
// Within a slice: workgroup b takes entries [256 c, 256 c + 256) for c = b, b + gridDim.x, ... until the slice's count is reached,
// an entry outside the frame is skipped, each lane stores its own 4 bytes (and its own float4); no LDS transpose.
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
    {  // stage the scene constants (portal matrices, uniforms) in LDS once per workgroup, as the slices render entry does
        const unsigned int* src = reinterpret_cast<const unsigned int*>(&glsl::ptl_u);
        unsigned int* dst = reinterpret_cast<unsigned int*>(&glsl::ptl_lds_u);
        for (int i = t; i < (int)(sizeof(glsl::ptl_uniform_block) / 4); i += 256) dst[i] = src[i];
        __syncthreads();
    }
#endif
    const unsigned int z = blockIdx.z;                                         // workgroup-uniform, like everything derived from it
    const glsl::ptl_uniform_block* const ptl_slice_block = ptl_slices + z;     // this slice's uniforms ...
    const unsigned int* const list = lists + (unsigned long long)z * list_stride;  // ... its list ...
    if (out_rgba8 != nullptr) out_rgba8 += (unsigned long long)z * ptl_slice_pixels;  // ... and its frame
    if (out_rgba32f != nullptr) out_rgba32f += 4ull * z * ptl_slice_pixels;
    const unsigned long long listed = counts[z];  // a scalar load; never read past the slice's own list, whatever the word holds
    const unsigned int n = (unsigned int)(listed < list_stride ? listed : list_stride);
    const unsigned int pixels = (unsigned int)width * (unsigned int)height;
    for (unsigned int first = blockIdx.x * 256u; first < n; first += gridDim.x * 256u) {
        const unsigned int i = first + (unsigned int)t;
        if (i >= n) continue;
        const unsigned int idx = list[i];
        if (idx >= pixels) continue;  // (never for a list the classification kernel wrote: a caller's own list stays inside the frame)
        const unsigned int py = idx / (unsigned int)width, px = idx - py * (unsigned int)width;
        const glsl::vec4 c = glsl::shade_pixel_in(glsl::vec2((float)px + 0.5f, (float)py + 0.5f), ptl_slice_block);
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

