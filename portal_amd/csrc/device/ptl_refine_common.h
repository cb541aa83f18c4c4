// ptl_refine_common.h -- adaptive anti-aliasing, pass 3 of 3: what every list-driven render entry runs.  Spliced in front of the entry
// itself (device/ptl_refine_entry.h for one frame; its sibling over the slices of a batch), the way kernels/aa_edges_common.h stands in
// front of the two classification kernels; a source generated without such an entry has no trace of it.
//
// `list` holds `n` pixel indices y * width + x of ONE frame, flagged by the classification kernel (kernels/aa_edges_common.h); they are
// read HERE, so the host never looks at them and nothing synchronises between the passes.  The grid has a fixed size chosen by the host;
// workgroup b takes entries [256 c, 256 c + 256) for c = b, b + gridDim.x, ... until `n` is reached -- a static stride, not a work queue.
// A wave takes 64 consecutive entries, which the classification kernel produced together (8x8 tile after 8x8 tile of one 64x32 region):
// still a compact bundle of rays.  Each lane shades its own pixel with `shade` -- the entry's way to call the tracer the render entry
// calls; a pixel's value does not depend on which lanes share its wave -- and stores its own 4 bytes (and its own float4): no LDS
// transpose, the lanes of a wave are not a rectangle.  Every argument is workgroup-uniform.
#if !defined(PTL_TELEPORT_MODULE)
template <typename Shade>
__device__ __forceinline__ void ptl_refine_walk(const unsigned int* __restrict__ list, unsigned int n,  // the entries, y * width + x each, and how many
                                                unsigned int* __restrict__ out_rgba8,                     // the full frame pass 1 wrote, or null
                                                float* __restrict__ out_rgba32f,                          // same, 4 floats per pixel, or null
                                                int width, int height,                                     // full frame size
                                                unsigned long long* __restrict__ segment_counter, Shade shade) {
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
    const unsigned int pixels = (unsigned int)width * (unsigned int)height;
    for (unsigned int first = blockIdx.x * 256u; first < n; first += gridDim.x * 256u) {
        const unsigned int i = first + (unsigned int)t;
        if (i >= n) continue;
        const unsigned int idx = list[i];
        if (idx >= pixels) continue;  // (never for a list the classification kernel wrote: a caller's own list stays inside the frame)
        const unsigned int py = idx / (unsigned int)width, px = idx - py * (unsigned int)width;
        const glsl::vec4 c = shade(glsl::vec2((float)px + 0.5f, (float)py + 0.5f));
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
