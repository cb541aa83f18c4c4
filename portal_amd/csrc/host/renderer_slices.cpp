// renderer_slices.cpp -- staged slices (renderer.h `StagedSlices`).
#include <algorithm>

#include "renderer.h"

namespace ptl {

// Slice j, if staged, lets go of its kernel's texel buffers -- unless that kernel is parked: it is destroyed with them in drop().
void StagedSlices::release_hold(size_t j) {
    if (!(mask >> j & 1u) || !kernels[j]) return;
    if (std::find(parked.begin(), parked.end(), kernels[j]) == parked.end()) ptl_kernel_hold_textures(kernels[j], 0);
}

int StagedSlices::stage(int index, ptl_kernel* kernel, int aa_count_now) {
    // kept as a snapshot of the kernel's host copy of the uniform block: the block layout is the scene's, not the build's, so the
    // snapshot outlives a rebuild of the kernel between two stage calls (a clip-constant build whose compiled-in value moved)
    if (blocks.size() < 16) blocks.resize(16);
    if (kernels.size() < 16) kernels.resize(16, nullptr);
    std::vector<unsigned char>& b = blocks[index];
    b.resize(ptl_kernel_uniform_block_size(kernel));
    int rc = ptl_kernel_snapshot_uniforms(kernel, b.data(), b.size());
    if (rc != PTL_OK) return rc;
    release_hold(index);  // staged twice: the earlier one is dropped
    // the block names the texel buffers bound NOW (a video texture may step before the next stage call): they stay until the launch
    ptl_kernel_hold_textures(kernel, 1);
    kernels[index] = kernel;
    aa_count[index] = aa_count_now;
    mask |= 1u << index;
    return PTL_OK;
}

bool StagedSlices::names(const ptl_kernel* k) const {
    for (size_t j = 0; j < kernels.size(); ++j)
        if ((mask >> j & 1u) && kernels[j] == k) return true;
    return false;
}

int StagedSlices::stage_run(ptl_kernel* k, int j0, int j1) {
    int rc = PTL_OK;
    for (int j = j0; j < j1 && rc == PTL_OK; ++j) rc = ptl_kernel_stage_slice_from(k, j - j0, blocks[j].data(), blocks[j].size());
    return rc;
}

void StagedSlices::drop() {
    for (size_t j = 0; j < kernels.size(); ++j) release_hold(j);
    mask = 0;
    for (ptl_kernel* k : parked) ptl_kernel_destroy(k);
    parked.clear();
}

}  // namespace ptl
