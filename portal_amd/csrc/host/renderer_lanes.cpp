// renderer_lanes.cpp -- concurrent draws (renderer.h `Lanes`).
#include <chrono>
#include <mutex>

#include "renderer.h"

namespace ptl {

// The lanes' streams are shared by every renderer of a process (per device, created on demand, never destroyed): the HIP runtime multiplexes
// streams onto a handful of hardware queues (four by default), and two streams that land on the same queue serialise.  A stream pair per
// renderer worked for the first renderer of a process and overlapped nothing for the fourth (bench.py's other workloads, round 6: 0.0364 ms
// per 1080p frame with and without lanes; 0.0304 when the same renderer was the first).  Draws of different renderers on one lane stream
// just follow each other.
static void* pooled_lane_stream(int device, size_t index) {
    static std::mutex guard;
    static std::map<int, std::vector<void*>> pool;
    std::lock_guard<std::mutex> lock(guard);
    std::vector<void*>& streams = pool[device];
    while (streams.size() <= index) {
        void* s = nullptr;
        if (ptl_stream_create(device, &s) != PTL_OK) return nullptr;
        streams.push_back(s);
    }
    return streams[index];
}

int Lanes::set_option(const std::string& n, double v) {
    if (n == "concurrent_draws") {  // 1 = off (the default); K <= 8 kernel instances on K internal streams
        int k = (int)v;
        if (k < 1 || k > 8) return PTL_ERR_INVALID;
        if (k != concurrent) {
            drop_clones();
            concurrent = k;
        }
        return PTL_OK;
    }
    if (n == "lane_stagger_us") {  // the first draw of lanes 2 .. K after a join comes this much (x 2 / K) later than the previous lane's
        if (!(v >= 0.0) || v > 1e6) return PTL_ERR_INVALID;
        lane_stagger_us = v;
        return PTL_OK;
    }
    if (n == "lane_fence") {  // 1 (default): a lane's launch waits for what the caller's stream holds; 0: it does not
        lane_fence = v > 0.5;
        return PTL_OK;
    }
    return PTL_UNKNOWN_UNIFORM;
}

// (a lane's `done` event is recorded when somebody asks -- here and in join -- not behind every launch: one packet less per draw)
void Lanes::wait() {
    lane_draws_since_join = 0;
    for (auto& l : lanes)
        if (l.busy && l.done) {
            if (ptl_event_record(l.done, l.stream) == PTL_OK) ptl_event_synchronize(l.done);
            l.busy = false;
        }
}
void Lanes::drop_clones() {
    wait();
    for (auto& l : lanes) {
        ptl_kernel_destroy(l.clone);
        l.clone = nullptr;
    }
    lanes_of = nullptr;
}
int Lanes::join(void* stream) {
    lane_draws_since_join = 0;
    for (auto& l : lanes)
        if (l.busy && l.done) {
            if (int rc = ptl_event_record(l.done, l.stream); rc != PTL_OK) return rc;
            if (int rc = ptl_stream_wait_event(stream, l.done); rc != PTL_OK) return rc;
            l.busy = false;
        }
    return PTL_OK;
}
Lanes::~Lanes() {
    drop_clones();
    for (auto& l : lanes)
        if (l.done) ptl_event_destroy(l.done);
    if (fence) ptl_event_destroy(fence);
}

// One draw of a renderer with "concurrent_draws" K > 1, issued on the caller's stream `stream` without a request for its time: it goes to
// the next of K lanes.  prepare_draw leaves the complete current state in the primary kernel's (`active`) host copy of the uniform block; a
// clone takes that copy over and uploads it behind its own previous launch, on its own stream.  The launch waits (GPU-side) for what the
// caller's stream has queued so far -- the consumer of this target buffer from the previous round -- and nothing waits for the launch
// until ptl_renderer_join.
int Lanes::draw(ptl_kernel* active, int device, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* stream) {
    if ((int)lanes.size() != concurrent) {
        drop_clones();
        for (auto& l : lanes)
            if (l.done) ptl_event_destroy(l.done);
        lanes.assign((size_t)concurrent, Lane{});
        for (size_t i = 0; i < lanes.size(); ++i) {
            Lane& l = lanes[i];
            l.stream = pooled_lane_stream(device, i);
            if (!l.stream) return PTL_ERR_HIP;
            if (int rc = ptl_event_create(device, &l.done); rc != PTL_OK) return rc;
        }
        if (!fence)
            if (int rc = ptl_event_create(device, &fence); rc != PTL_OK) return rc;
    }
    if (lanes_of != active) {  // first use, or the kernel was rebuilt / switched: instances of THIS code object
        drop_clones();
        for (size_t i = 1; i < lanes.size(); ++i)
            if (int rc = ptl_kernel_clone(active, &lanes[i].clone); rc != PTL_OK) return rc;
        lanes_of = active;
    }
    const size_t idx = next_lane++ % lanes.size();
    Lane& lane = lanes[idx];
    ptl_kernel* k = idx == 0 ? active : lane.clone;
    if (idx != 0)
        if (int rc = ptl_kernel_copy_uniforms(k, active); rc != PTL_OK) return rc;
    if (lane_fence) {
        if (int rc = ptl_event_record(fence, stream); rc != PTL_OK) return rc;
        if (int rc = ptl_stream_wait_event(lane.stream, fence); rc != PTL_OK) return rc;
    }
    if (lane_stagger_us > 0.0 && lane_draws_since_join >= 1 && lane_draws_since_join < lanes.size()) {
        const auto until = std::chrono::steady_clock::now() + std::chrono::nanoseconds((long long)(lane_stagger_us * 2000.0 / (double)lanes.size()));
        while (std::chrono::steady_clock::now() < until) {
        }
    }
    ++lane_draws_since_join;
    if (int rc = ptl_kernel_render(k, frame, out_rgba8, out_rgba32f, nullptr, lane.stream, nullptr); rc != PTL_OK) return rc;
    lane.busy = true;
    return PTL_OK;
}

}  // namespace ptl
