// renderer_camera.cpp -- the renderer's camera (renderer.h `Camera`) and how it moves through portals.
//   RotateAroundCam::get_matrix          src/main.rs:278-304   -> Camera::matrix()
//   SceneRenderer::teleport_camera       src/main.rs:1217-1264 -> teleport_camera()
//   SceneRenderer::teleport_eye_matrices src/main.rs:1121-1172 -> teleport_eye_matrices()
//   SceneRenderer::update                src/main.rs:1430-1538 -> ptl_renderer_update
#include <cstdlib>
#include <optional>

#include "renderer.h"

using namespace ptl;

namespace ptl {

DVec3 cam_pos(const Camera& c) {  // RotateAroundCam::get_cam_pos (src/main.rs:316-318)
    DVec4 p = c.matrix().mul_vec4(DVec4(0.0, 0.0, 0.0, 1.0));
    return DVec3(p.x, p.y, p.z);
}

double calc_scale(const DMat4& m) {  // src/main.rs:1325-1333
    return (m.c[0].length() + m.c[1].length() + m.c[2].length()) / 3.0;
}

// The three camera matrices as the kernel gets them (binary32): bottom row 0 0 0 1?  (RotateAroundCam::get_matrix builds an affine basis,
// src/main.rs:278-304; the accumulated portal matrix in front of it is affine while the portals are.)
bool camera_is_affine(const ptl_renderer& r) {
    float f[16];
    r.cam.matrix().to_f32(f);
    if (!matrix_is_affine(f)) return false;
    if (r.opt.draw_side_by_side || r.opt.draw_anaglyph) {
        r.cam.left_eye_matrix.to_f32(f);
        if (!matrix_is_affine(f)) return false;
        r.cam.right_eye_matrix.to_f32(f);
        if (!matrix_is_affine(f)) return false;
    }
    return true;
}

CalculatedCam calculated_of(const Camera& c) {  // RotateAroundCam::get_calculated_cam (src/main.rs:156-167)
    CalculatedCam out;
    out.look_at = c.look_at;
    out.alpha = c.alpha;
    out.beta = c.beta;
    out.r = c.r;
    out.in_subspace = c.in_subspace;
    out.free_movement = c.free_movement;
    out.matrix = c.teleport_matrix;
    return out;
}
CalculatedCam calculated_of(const CamSettings& c) {  // the scene's `cam` block: the original camera, teleport matrix = I (RotateAroundCam::set_cam)
    CalculatedCam out;
    out.look_at = c.look_at;
    out.alpha = c.alpha;
    out.beta = c.beta;
    out.r = c.r;
    return out;
}

static bool same_matrix(const DMat4& a, const DMat4& b) {
    for (int k = 0; k < 4; ++k)
        if (a.c[k].x != b.c[k].x || a.c[k].y != b.c[k].y || a.c[k].z != b.c[k].z || a.c[k].w != b.c[k].w) return false;
    return true;
}

// `send_camera_object_matrix` (src/main.rs:147,1432-1436,1530-1534): Matrix::Camera evaluates to the camera's matrix
void send_camera_matrix(ptl_renderer* r) {
    DMat4 m = r->cam.matrix();
    if (!same_matrix(m, r->scene->camera_matrix)) {
        r->scene->camera_matrix = m;
        ++r->scene->version;
    }
}

// SceneRenderer::teleport_external_ray as Option<DVec3> + flags
struct RayQuery {
    bool teleported = false, hit_object = false, changed_subspace = false;
    DVec3 pos;
};
static int query_ray(ptl_renderer* r, const DVec3& a, const DVec3& b, RayQuery* q) {
    double pa[3] = {a.x, a.y, a.z}, pb[3] = {b.x, b.y, b.z}, out[3] = {0, 0, 0};
    int hit = 0, sub = 0, tel = 0;
    int rc = ptl_renderer_teleport_ray(r, pa, pb, out, &hit, &sub, &tel);
    if (rc != PTL_OK) return rc;
    q->teleported = tel != 0;
    q->hit_object = hit != 0;
    q->changed_subspace = sub != 0;
    q->pos = DVec3(out[0], out[1], out[2]);
    return PTL_OK;
}

// SceneRenderer::teleport_matrix (src/main.rs:1174-1215): finite-difference Jacobian of the portal map
// around the camera, three more ray queries with +-dx offsets along the camera's axes.
static int teleport_matrix(ptl_renderer* r, const DMat4& matrix, const DVec3& start_pos, const DVec3& direction_pos, const DVec3& actual, double dx,
                    bool* ok, DMat4* out) {
    *ok = false;
    DVec4 cols[3];
    const DVec4 axes[3] = {DVec4(1, 0, 0, 0), DVec4(0, 1, 0, 0), DVec4(0, 0, 1, 0)};
    for (int k = 0; k < 3; ++k) {
        DVec4 v4 = matrix.mul_vec4(axes[k]) * dx;
        DVec3 v(v4.x, v4.y, v4.z);
        RayQuery q;
        int rc = query_ray(r, start_pos + v, direction_pos + v, &q);
        if (rc != PTL_OK) return rc;
        if (!q.teleported) return PTL_OK;  // `?` on None
        DVec3 d = q.pos - actual;
        cols[k] = DVec4(d.x / dx, d.y / dx, d.z / dx, 0.0);  // DVec4::from((i, 0.)) / dx
    }
    DMat4 new_mat = DMat4::from_cols(cols[0], cols[1], cols[2], DVec4(0, 0, 0, 1));
    DVec4 moved = (new_mat * matrix.inverse()).mul_vec4(DVec4(direction_pos.x, direction_pos.y, direction_pos.z, 1.0));
    DVec3 pos = actual - DVec3(moved.x, moved.y, moved.z);
    *out = DMat4::from_cols(cols[0], cols[1], cols[2], DVec4(pos.x, pos.y, pos.z, 1.0));
    *ok = true;
    return PTL_OK;
}

// SceneRenderer::teleport_camera (src/main.rs:1217-1264)
static int teleport_camera(ptl_renderer* r, const Camera& prev_cam, int* teleported, int* blocked) {
    Camera& cam = r->cam;
    if (cam.do_not_teleport_one_frame) {
        cam.do_not_teleport_one_frame = false;
        cam.prev_cam_pos = cam_pos(cam);
        return PTL_OK;
    }
    if (!(cam.allow_teleport || cam.stop_at_objects)) return PTL_OK;
    DVec3 pos = cam_pos(cam);
    RayQuery q;
    int rc = query_ray(r, cam.prev_cam_pos, pos, &q);
    if (rc != PTL_OK) return rc;
    if (cam.stop_at_objects && q.hit_object) {
        cam = prev_cam;
        if (blocked) *blocked = 1;
        return PTL_OK;
    }
    if (!q.teleported) {
        cam.prev_cam_pos = pos;
        return PTL_OK;
    }
    if (!cam.allow_teleport) return PTL_OK;
    for (double dx : {0.001, 0.0001, 0.00001, 0.000001}) {
        bool ok = false;
        DMat4 m;
        rc = teleport_matrix(r, cam.teleport_matrix, cam.prev_cam_pos, pos, q.pos, dx, &ok, &m);
        if (rc != PTL_OK) return rc;
        if (!ok) continue;
        cam.teleport_matrix = m;
        if (q.changed_subspace) cam.in_subspace = !cam.in_subspace;
        cam.prev_cam_pos = cam_pos(cam);
        if (teleported) *teleported = 1;
        return PTL_OK;
    }
    cam = prev_cam;  // no step size produced a Jacobian: stay where we were
    if (blocked) *blocked = 1;
    return PTL_OK;
}

// SceneRenderer::teleport_eye_matrices (src/main.rs:1121-1172): each eye sits eye_distance to the side of the camera; if
// the segment camera -> eye crosses a portal, the eye gets its own teleported matrix (and subspace flag).
static int teleport_eye_matrices(ptl_renderer* r) {
    Camera& cam = r->cam;
    if (!((r->opt.draw_anaglyph || r->opt.draw_side_by_side) && cam.allow_teleport)) return PTL_OK;
    double eye_distance = r->opt.swap_eyes ? -r->opt.eye_distance : r->opt.eye_distance;
    auto one_eye = [&](double x, DMat4* out_m, bool* out_sub) -> int {
        DVec3 start_pos = cam_pos(cam);
        DMat4 m = cam.matrix();
        DVec4 d4 = m.mul_vec4(DVec4(x, 0.0, 0.0, 1.0));
        DVec3 direction_pos(d4.x, d4.y, d4.z);
        DVec3 shift = direction_pos - start_pos;
        DMat4 translation = DMat4::from_cols({1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {shift.x, shift.y, shift.z, 1});
        *out_m = translation * m;
        *out_sub = cam.in_subspace;
        RayQuery q;
        int rc = query_ray(r, start_pos, direction_pos, &q);
        if (rc != PTL_OK) return rc;
        if (!q.teleported) return PTL_OK;
        for (double dx : {0.001, 0.0001, 0.00001, 0.000001}) {
            bool ok = false;
            DMat4 tm;
            rc = teleport_matrix(r, *out_m, start_pos, direction_pos, q.pos, dx, &ok, &tm);
            if (rc != PTL_OK) return rc;
            if (!ok) continue;
            *out_m = tm;
            if (q.changed_subspace) *out_sub = !cam.in_subspace;
            break;
        }
        return PTL_OK;
    };
    int rc = one_eye(-eye_distance, &cam.left_eye_matrix, &cam.left_eye_in_subspace);
    if (rc == PTL_OK) rc = one_eye(eye_distance, &cam.right_eye_matrix, &cam.right_eye_in_subspace);
    return rc;
}

}  // namespace ptl

extern "C" int ptl_renderer_set_camera(ptl_renderer* r, const double look_at[3], double alpha, double beta, double radius) {
    if (!r || !look_at) return PTL_ERR_INVALID;
    r->cam.look_at = DVec3(look_at[0], look_at[1], look_at[2]);
    r->cam.alpha = alpha;
    r->cam.beta = beta;
    r->cam.r = radius;
    r->cam.prev_cam_pos = cam_pos(r->cam);  // placing the camera is not a move: no portal crossing is looked for
    ++r->options_version;
    return PTL_OK;
}

extern "C" int ptl_renderer_use_camera(ptl_renderer* r, const char* camera) {
    if (!r || !camera) return PTL_ERR_INVALID;
    return guarded([&] {
        std::string name = camera;
        ++r->options_version;
        if (name.empty()) {  // original camera: scene.cam, teleport matrix = I (RotateAroundCam::set_cam)
            r->cam.take(calculated_of(r->scene->cam));
            r->cam.from = r->scene->current_cam = -1;
            return PTL_OK;
        }
        int idx = name[0] == '#' ? std::atoi(name.c_str() + 1) : r->scene->find_camera(name);
        if (idx < 0 || idx >= (int)r->scene->cameras.size()) return 1;
        auto to = r->scene->calculated_cam(r->scene->cameras[idx]);
        if (!to) return 1;
        if (r->cam.from < 0) r->original_cam = calculated_of(r->cam);
        r->cam.take(*to);  // SceneRenderer::update (src/main.rs:1465-1477)
        if (r->cam.free_movement) r->cam.look_at = r->cam.pos_vec() + r->cam.look_at;
        r->cam.from = r->scene->current_cam = idx;
        r->cam.do_not_teleport_one_frame = true;
        return PTL_OK;
    });
}

extern "C" int ptl_renderer_move_camera(ptl_renderer* r, const double look_at[3], double alpha, double beta, double radius, int* teleported,
                                        int* blocked) {
    if (!r || !look_at) return PTL_ERR_INVALID;
    if (teleported) *teleported = 0;
    if (blocked) *blocked = 0;
    return guarded([&] {
        Camera prev = r->cam;
        r->cam.look_at = DVec3(look_at[0], look_at[1], look_at[2]);
        r->cam.alpha = alpha;
        r->cam.beta = beta;
        r->cam.r = radius;
        ++r->options_version;
        int rc = teleport_camera(r, prev, teleported, blocked);
        if (rc == PTL_OK) rc = teleport_eye_matrices(r);
        ++r->options_version;
        return rc;
    });
}

// SceneRenderer::update (src/main.rs:1430-1538): the per-frame step of the video pipeline and of render-frame
extern "C" int ptl_renderer_update(ptl_renderer* r, double seconds, int* teleported, int* blocked) {
    if (!r) return PTL_ERR_INVALID;
    if (teleported) *teleported = 0;
    if (blocked) *blocked = 0;
    return guarded([&] {
        Scene& scene = *r->scene;
        Camera& cam = r->cam;
        if (!r->has_prev_cam) {  // SceneRenderer::new: prev_cam = cam.clone()
            r->prev_cam = cam;
            r->has_prev_cam = true;
        }
        ++r->options_version;
        std::optional<CalculatedCam> override_cam = scene.update(seconds);
        send_camera_matrix(r);

        int current_cam = scene.current_cam;
        if (cam.from != current_cam) {
            CalculatedCam c;
            if (current_cam >= 0) {
                if (cam.from < 0) r->original_cam = calculated_of(cam);
                auto got = scene.calculated_cam(scene.cameras.at(current_cam));
                if (!got) throw SceneError("camera can't be evaluated");
                c = *got;
            } else {
                c = r->original_cam;
            }
            cam.from = current_cam;
            cam.take(c);
            if (cam.free_movement) cam.look_at = cam.pos_vec() + cam.look_at;
            cam.do_not_teleport_one_frame = true;
        } else if (cam.from >= 0) {
            auto got = scene.calculated_cam(scene.cameras.at(cam.from));
            if (!got) throw SceneError("camera can't be evaluated");
            if (!cam.free_movement) cam.look_at = got->look_at;
        }

        if (override_cam) {
            cam.take(*override_cam, override_cam->override_matrix);
            if (override_cam->override_matrix) cam.do_not_teleport_one_frame = true;
        }

        int rc = PTL_OK;
        if (!same_matrix(cam.matrix(), r->prev_cam.matrix())) {
            Camera prev = r->prev_cam;
            rc = teleport_camera(r, prev, teleported, blocked);
        }
        if (rc == PTL_OK) rc = teleport_eye_matrices(r);
        r->prev_cam = cam;
        send_camera_matrix(r);
        ++r->options_version;
        if (rc == PTL_OK) rc = update_videos(r);
        return rc;
    });
}

extern "C" int ptl_renderer_camera_state(ptl_renderer* r, double teleport16[16], int* in_subspace, double position[3]) {
    if (!r) return PTL_ERR_INVALID;
    if (teleport16) r->cam.teleport_matrix.to_cols_array(teleport16);
    if (in_subspace) *in_subspace = r->cam.in_subspace ? 1 : 0;
    if (position) {
        DVec3 p = cam_pos(r->cam);
        position[0] = p.x;
        position[1] = p.y;
        position[2] = p.z;
    }
    return PTL_OK;
}
