// internal.h -- shared between the translation units of libportal_amd.so.
#pragma once
#include <string>

namespace ptl {
void set_last_error(const std::string& msg);
extern thread_local std::string g_last_error;
// codegen.cpp.  Bottom row exactly 0 0 0 1 (column-major elements 3, 7, 11, 15), or NaN in every element (a switched-off object: its products are
// NaN whatever the w): what a kernel with affine rays asks of every scene matrix -- at generation time, before every upload of the renderer
// (renderer_builds.cpp `zero_patterns_broken`) and of a layer-1 caller (kernel.cpp `ptl_kernel_set_uniform`).
bool matrix_keeps_rays_affine(const float m[16]);
}  // namespace ptl
