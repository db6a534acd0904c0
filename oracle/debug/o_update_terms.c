/*
 * oracle/debug/o_update_terms.c -- TEST INFRASTRUCTURE (CPU oracle), stage export for tests/test_update_crafted_host.py.
 *
 * The fp32 intermediates that K9 (o_map.c: o_k9_update, update_surfels.vert:140-217) compares, per surfel, formed with the
 * oracle's own helpers (o_math.h, o_ctx.h) in K9's operation order: x01 * W and y01 * H before the floor, imz, the
 * front-face product, and -- where both texels are valid -- distance and angle.  It reads the context (parameters, pose
 * table) and changes nothing; it lives beside the oracle proper, not in it, so that the arithmetic specification
 * (the .c and .h files of oracle/ itself, whose hash the recorded 4541-scan trace carries) stays untouched.  The host
 * test pins these terms to what o_k9_update itself decided (matched surfels, marked pixels) on every room scene.
 *
 * Not exported here, and read by the test from the update's own results instead: new_radius (the radius_conf map at the
 * texel these coordinates name) and the confidence before the cap (the confidence of the SURVIVING records below the cap).
 * The confidence bound is therefore measured on survivors only: a surfel that the update deletes -- the far side of
 * log_unstable -- contributes nothing to it.
 */
#include "../o_ctx.h"

void ora_debug_update_terms(const ora_ctx* c, const suma_surfel* surfels, uint32_t n, const float pose[16],
                            const ora_frame* f, float* terms /* n x 6, preset by the caller */) {
  const suma_params* p = &c->p;
  const ora_proj q = o_proj_data(p);
  const int32_t W = (int32_t)p->data_width, H = (int32_t)p->data_height;
  float inv_pose[16];
  om4_rigid_inverse(pose, inv_pose);
  for (uint32_t i = 0; i < n; ++i) {
    const suma_surfel in = surfels[i];
    const int32_t creation_timestamp = (int32_t)in.count;
    /* the update sets poses[timestamp] = pose before anything reads the table */
    const float* Ps = ((uint32_t)creation_timestamp == c->timestamp) ? pose : c->poses + 16 * (size_t)creation_timestamp;
    ov3 old_position = om4_point(Ps, ov3_make(in.x, in.y, in.z));
    ov3 old_normal = om4_dir(Ps, ov3_make(in.nx, in.ny, in.nz));
    ov3 vertex = om4_point(inv_pose, old_position);
    ov3 normal = ov3_normalize(om4_dir(inv_pose, old_normal));
    float* t = terms + 6 * (size_t)i;
    ov3 pr = o_project01(&q, vertex);
    t[0] = pr.x * q.width;
    t[1] = pr.y * q.height;
    t[2] = pr.z;
    t[3] = ov3_dot(normal, ov3_divs(ov3_neg(vertex), ov3_len(vertex)));
    float imx = sdm_floor(t[0]) + 0.5f, imy = sdm_floor(t[1]) + 0.5f;
    int in_tex = (imx >= 0.0f && imx < q.width && imy >= 0.0f && imy < q.height);
    int32_t tx = in_tex ? (int32_t)sdm_floor(imx) : -1, ty = in_tex ? (int32_t)sdm_floor(imy) : -1;
    suma_float4 dv = o_texel(f->vertex, W, H, tx, ty), dn = o_texel(f->normal, W, H, tx, ty);
    if (!((dv.w > 0.5f) && (dn.w > 0.5f))) continue;
    ov3 v = ov3_make(dv.x, dv.y, dv.z), nn = ov3_make(dn.x, dn.y, dn.z);
    ov3 v_global = om4_point(pose, v);
    ov3 n_global = ov3_normalize(om4_dir(pose, nn));
    t[4] = fabsf(ov3_dot(old_normal, ov3_sub(v_global, old_position)));
    t[5] = ov3_len(ov3_cross(n_global, old_normal));
  }
}
