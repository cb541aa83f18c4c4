# Builds libportal_amd.so (C ABI, include/portal_amd.h), the CLI and the fixed gfx950 helpers.
#   make            -> portal_amd/libportal_amd.so + portal_amd/portal-amd
#   make kernels    -> portal_amd/kernels/*.hsaco (hipcc --genco, gfx950)
CXX      ?= g++
HIPCC    ?= /opt/rocm/bin/hipcc
CXXFLAGS ?= -O2 -g -std=c++20 -fPIC -Wall -Wextra -Wno-unused-parameter
HOST     := portal_amd/csrc/host
DEVICE   := portal_amd/csrc/device
OBJDIR   := build/obj
SRCS     := ron.cpp formula.cpp scene.cpp glsl_tokens.cpp glsl_translate.cpp glsl_aliasing.cpp glsl_bound.cpp glsl_syntax.cpp glsl_binding.cpp glsl_hoist.cpp glsl_affine.cpp glsl_masks.cpp codegen.cpp embedded.cpp hip_api.cpp kernel.cpp postprocess.cpp png_io.cpp capi.cpp capi_tools.cpp renderer_builds.cpp renderer_camera.cpp renderer_draw.cpp renderer_lanes.cpp renderer_slices.cpp multigpu.cpp
OBJS     := $(SRCS:%.cpp=$(OBJDIR)/%.o)
LIB      := portal_amd/libportal_amd.so
CLI      := portal_amd/portal-amd
KERNELS  := portal_amd/kernels/fb_store.hsaco portal_amd/kernels/average_images.hsaco portal_amd/kernels/yuv10.hsaco portal_amd/kernels/yuv10_f32.hsaco portal_amd/kernels/rgb48_f32.hsaco portal_amd/kernels/aa_edges.hsaco portal_amd/kernels/aa_edges_slices.hsaco portal_amd/kernels/pass_stats.hsaco portal_amd/kernels/pass_gray16.hsaco portal_amd/kernels/pass_slices_gray16.hsaco portal_amd/kernels/png_deflate.hsaco portal_amd/kernels/png_huffman.hsaco

all: $(LIB) $(CLI)

$(HOST)/embedded_device_sources.inc: $(DEVICE)/ptl_glsl.h $(DEVICE)/ptl_library.h $(DEVICE)/ptl_trace.tpl $(DEVICE)/ptl_entry.h $(DEVICE)/ptl_refine_common.h $(DEVICE)/ptl_refine_entry.h $(DEVICE)/ptl_refine_slices_entry.h portal_amd/csrc/embed_sources.py
	python3 portal_amd/csrc/embed_sources.py $@ device_source_glsl=$(DEVICE)/ptl_glsl.h device_source_library=$(DEVICE)/ptl_library.h \
	    device_source_trace_template=$(DEVICE)/ptl_trace.tpl device_source_entry=$(DEVICE)/ptl_entry.h device_source_refine_entry=$(DEVICE)/ptl_refine_common.h+$(DEVICE)/ptl_refine_entry.h \
	    device_source_refine_slices_entry=$(DEVICE)/ptl_refine_common.h+$(DEVICE)/ptl_refine_slices_entry.h

$(OBJDIR)/embedded.o: $(HOST)/embedded_device_sources.inc
$(OBJDIR)/%.o: $(HOST)/%.cpp $(wildcard $(HOST)/*.h) include/portal_amd.h portal_amd/csrc/kernels/yuv_shape.h portal_amd/csrc/kernels/rgb48_shape.h portal_amd/csrc/kernels/pass_key.h portal_amd/csrc/kernels/png_deflate_shape.h
	@mkdir -p $(OBJDIR)
	$(CXX) $(CXXFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	$(CXX) -shared -o $@ $(OBJS) -ldl -lz -lpthread

$(CLI): $(HOST)/cli.cpp $(HOST)/cli_video.cpp $(wildcard $(HOST)/cli*.h) $(LIB) include/portal_amd.h
	$(CXX) $(CXXFLAGS) $(HOST)/cli.cpp $(HOST)/cli_video.cpp -o $@ -Lportal_amd -lportal_amd -Wl,-rpath,'$$ORIGIN'

kernels: $(KERNELS)
portal_amd/kernels/%.hsaco: portal_amd/csrc/kernels/%.hip portal_amd/csrc/kernels/average_common.h portal_amd/csrc/kernels/yuv_common.h portal_amd/csrc/kernels/yuv_shape.h portal_amd/csrc/kernels/rgb48_shape.h portal_amd/csrc/kernels/aa_edges_common.h portal_amd/csrc/kernels/pass_key.h portal_amd/csrc/kernels/png_deflate_shape.h portal_amd/csrc/kernels/png_deflate_common.h
	@mkdir -p portal_amd/kernels
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -mllvm -vgpr-regalloc=basic --genco --no-gpu-bundle-output $< -o $@  # allocator: see kernel.cpp

clean:
	rm -rf build $(LIB) $(CLI) portal_amd/kernels $(HOST)/embedded_device_sources.inc

.PHONY: all kernels clean
