// shf_render.hip -- camera sensors (ABI v16; warped trimesh v20): one ray per pixel against the analytic collision shapes
// of each env, the ground plane, the height field or the warped trimesh.  No rasteriser: boxes, spheres, capsules and
// convex polytopes are intersected in closed form, the height field by a 2-D DDA walk over its cells (two triangles each,
// split as the collision code splits them: along (i+1, j)-(i, j+1)).  The warped trimesh (ShfTerrain.warped, the mesh
// convert_heightfield_to_trimesh makes: shifted vertices, vertical risers, cells split along (i, j)-(i+1, j+1)) takes
// the same walk, testing in each cell the triangles of the cells whose hint bits say they reach into it (TW form, the kernel
// k_render_cameras_tw).  Conventions and constants: include/shifu_amd.h (ShfRenderScene); the checkers are tests/render_ref.py
// and tests/trimesh_render_ref.py, independent float64 brute-force casters.
//
// Layout: one 256-thread workgroup per (env, 16 x 16 pixel tile), a wave per 16 x 4 pixel strip.  The env's shape
// world poses are built once per workgroup into LDS (one thread per shape); each wave then culls the shapes' bounding
// spheres against the cone of its strip's rays (one lane per shape, a ballot), so the loop over candidate shapes is
// wave-uniform and its LDS reads are broadcasts.  Stores are one dword per lane per image, 64 consecutive bytes per row.
//
// Optical flow (FLOW form, kernels k_render_cameras_flow / k_render_cameras_tw_flow behind shf_render_cameras_flow): the
// caster knows the surface point X = o + s d and the body b behind every pixel, so ground-truth flow is one rigid transform
// and one projection per pixel.  The point as it was at the previous flow render is X' = p_b' + R_b' R_b^T (X - p_b) (primed:
// the previous render's body pose; the terrain is static, X' = X); projected into the previous camera pose (o', q') with the
// pixel-ray convention above: z' = fwd'.(X' - o'), x' = right'.(X' - o') / (z' t), y' = up'.(X' - o') / (z' t H/W),
// c' = (x' + 1) W/2 - 1/2, r' = (1 - y') H/2 - 1/2, and flow = (c - c', r - r') in pixels, u to the right, v downwards --
// the backward-looking motion vector, where the point is now minus where it was.  Flow is exactly +0.0 where nothing is
// hit, where z' <= 0 or a term is not finite, where prev_valid[env] == 0, and where neither the hit body's pose (7 floats,
// compared as bits) nor the camera's changed bits since the previous render (a static scene is exactly zero, not float32
// noise).  The integer image is Isaac Gym's encoding, q_u = sat16(rint(u 32768 / W)), q_v = sat16(rint(v 32768 / H)), u in
// the low half of the pixel's dword.  Isaac Gym's own sign and direction conventions are a closed binary: no parity with
// it is claimed.  The staging phase also builds, per shape, the body's motion transform Rm = R_b' R_b^T and tm (12 floats in
// a second LDS table, 3 KB) RELATIVE TO THE CAMERA ORIGIN o -- X' - o = Rm (X - o) + tm, tm = (p_b' - o) - Rm (p_b - o) --
// because envs sit tens of metres out on the terrain and X' - X is a small difference; and a per-shape `moved` flag.  The
// per-pixel flow work comes after the nearest hit is chosen (one 3 x 3 transform, three dot products), not in the candidate
// loop; depth / segmentation / color come from the same cast and are bit-equal to the plain kernels'.  The checker is
// tests/flow_ref.py.
//
// World view (kernels k_render_world / k_render_world_tw behind shf_render_world, at the end of this file): one camera that
// sees many envs, each displaced by an offset -- the headless viewer.  Same rays, intersections, walk and shading.
//
// Ray caster (kernels k_raycast / k_raycast_tw behind shf_raycast, and k_camera_points behind shf_camera_points, after the
// world view): arbitrary rays per env -- height scanners, lidars -- through the same intersections and walk, the ray
// parameter being the Euclidean range; and the point behind every pixel of a rendered depth image.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/shifu_amd.h"

int shf_set_error(const std::string& msg);   // shf_api.hip

#define RT_TILE 16
#define RT_THREADS 256
#define RT_SW 20   // floats per shape in LDS: c[3] R[9] param[3] radius col[3] pad
#define RT_MW 12   // FLOW: floats per shape in the motion table: Rm[9] tm[3]

namespace {

__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// row-major rotation of the unit quaternion (x, y, z, w)
__device__ __forceinline__ void quat_mat(const float* q, float* R) {
  const float x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - z * w);        R[2] = 2.0f * (x * z + y * w);
  R[3] = 2.0f * (x * y + z * w);        R[4] = 1.0f - 2.0f * (x * x + z * z); R[5] = 2.0f * (y * z - x * w);
  R[6] = 2.0f * (x * z - y * w);        R[7] = 2.0f * (y * z + x * w);        R[8] = 1.0f - 2.0f * (x * x + y * y);
}

// entry parameter of a sphere of radius r at the origin (INFINITY: missed); *n the outward unit normal there
__device__ __forceinline__ float hit_sphere(const float* o, const float* d, float r, float* n) {
  const float a = dot3(d, d), b = dot3(o, d), c = dot3(o, o) - r * r;
  const float disc = b * b - a * c;
  if (disc < 0.0f) return INFINITY;
  const float s = (-b - sqrtf(disc)) / a;
  const float ir = 1.0f / r;
  for (int k = 0; k < 3; k++) n[k] = (o[k] + s * d[k]) * ir;
  return s;
}

__device__ __forceinline__ float hit_box(const float* o, const float* d, const float* h, float* n) {
  float sin_ = -INFINITY, sout = INFINITY;
  int ax = 0;
  for (int k = 0; k < 3; k++) {
    const float inv = 1.0f / d[k];
    const float t1 = (-h[k] - o[k]) * inv, t2 = (h[k] - o[k]) * inv;
    const float tn = fminf(t1, t2), tf = fmaxf(t1, t2);
    if (tn > sin_) { sin_ = tn; ax = k; }
    sout = fminf(sout, tf);
  }
  if (!(sin_ <= sout)) return INFINITY;
  for (int k = 0; k < 3; k++) n[k] = 0.0f;
  n[ax] = d[ax] > 0.0f ? -1.0f : 1.0f;
  return sin_;
}

// capsule along local z: the segment [-hl, hl], radius r -- the first entry into the cylinder or either end sphere
__device__ __forceinline__ float hit_capsule(const float* o, const float* d, float r, float hl, float* n) {
  float best = INFINITY;
  const float a = d[0] * d[0] + d[1] * d[1];
  if (a > 0.0f) {
    const float b = o[0] * d[0] + o[1] * d[1], c = o[0] * o[0] + o[1] * o[1] - r * r;
    const float disc = b * b - a * c;
    if (disc >= 0.0f) {
      const float s = (-b - sqrtf(disc)) / a;
      const float z = o[2] + s * d[2];
      if (fabsf(z) <= hl) {
        best = s;
        n[0] = (o[0] + s * d[0]) / r; n[1] = (o[1] + s * d[1]) / r; n[2] = 0.0f;
      }
    }
  }
  for (int e = 0; e < 2; e++) {
    const float oc[3] = {o[0], o[1], o[2] - (e ? hl : -hl)};
    float ns[3];
    const float s = hit_sphere(oc, d, r, ns);
    if (s < best) { best = s; n[0] = ns[0]; n[1] = ns[1]; n[2] = ns[2]; }
  }
  return best;
}

__device__ __forceinline__ float hit_poly(const ShfRenderPoly* __restrict__ P, const float* o, const float* d, float* n) {
  float sin_ = -INFINITY, sout = INFINITY;
  int face = -1;
  const int nf = min(P->nf, SHF_RENDER_POLY_MAX_FACES);
  for (int f = 0; f < nf; f++) {
    const float pn[3] = {P->plane[f][0], P->plane[f][1], P->plane[f][2]};
    const float dn = dot3(pn, d), num = P->plane[f][3] - dot3(pn, o);
    if (dn < 0.0f) {
      const float s = num / dn;
      if (s > sin_) { sin_ = s; face = f; }
    } else if (dn > 0.0f) {
      sout = fminf(sout, num / dn);
    } else if (num < 0.0f) {
      return INFINITY;
    }
  }
  if (face < 0 || !(sin_ <= sout)) return INFINITY;
  n[0] = P->plane[face][0]; n[1] = P->plane[face][1]; n[2] = P->plane[face][2];
  return sin_;
}

// the plane of the height-field triangle v0 v1 v2 (world coordinates) when the ray meets its front face (upward normal):
// *s_out its parameter, n the unit normal; whether the hit lies inside the triangle is tested by the caller in cell units
__device__ __forceinline__ bool hf_triangle(const float* o, const float* d, const float* v0, const float* v1, const float* v2,
                                            float* s_out, float* n) {
  const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
  const float c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const float dn = dot3(c, d);
  if (!(dn < 0.0f)) return false;
  const float w[3] = {v0[0] - o[0], v0[1] - o[1], v0[2] - o[2]};
  *s_out = dot3(w, c) / dn;
  const float il = 1.0f / sqrtf(dot3(c, c));
  n[0] = c[0] * il; n[1] = c[1] * il; n[2] = c[2] * il;
  return true;
}

// One triangle of the warped mesh (world coordinates) against the ray: a hit counts on the front face (the side of
// (v1 - v0) x (v2 - v0)), inside the triangle in 3-D (risers have no extent in xy) and inside the walked cell's closed
// square [x0, x0 + hs] x [y0, y0 + hs], both with the walk's slack.  Collapsed triangles (zero area) are skipped.
__device__ __forceinline__ void tw_triangle(const float* o, const float* d, const float* v0, const float* v1, const float* v2,
                                            float s_min, float s_max, float x0, float y0, float ih, float* best, float* n) {
  const float eps = 1e-5f;
  const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
  const float c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const float dn = dot3(c, d), cc = dot3(c, c);
  if (!(dn < 0.0f) || !(cc > 1e-16f)) return;
  const float w[3] = {v0[0] - o[0], v0[1] - o[1], v0[2] - o[2]};
  const float idn = 1.0f / dn;
  const float s = dot3(w, c) * idn;
  if (!(s >= s_min && s <= s_max && s < *best)) return;
  // barycentric weights of v1 and v2 (Moeller-Trumbore, from the ray origin: no hit point is formed)
  const float pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
  const float qv[3] = {w[1] * e1[2] - w[2] * e1[1], w[2] * e1[0] - w[0] * e1[2], w[0] * e1[1] - w[1] * e1[0]};
  const float bu = dot3(w, pv) * idn, bv = dot3(d, qv) * idn;
  if (!(bu >= -eps && bv >= -eps && bu + bv <= 1.0f + eps)) return;
  const float u = (o[0] + s * d[0] - x0) * ih, v = (o[1] + s * d[1] - y0) * ih;
  if (!(u >= -eps && u <= 1.0f + eps && v >= -eps && v <= 1.0f + eps)) return;
  const float il = 1.0f / sqrtf(cc);
  *best = s;
  n[0] = c[0] * il; n[1] = c[1] * il; n[2] = c[2] * il;
}

// nearest front-facing surface of the warped mesh inside cell (i0, j0)'s closed square, s in [s_min, s_max]: the cell's
// own two triangles and those of the neighbouring rows / columns its hint bits name (bits 4-7 of the cell's byte,
// warp_map_from_shifts: every triangle whose horizontal projection meets the closed square, risers standing on its
// boundary included -- the set does not depend on the direction of the query, so it serves rays as it serves the
// collision code's vertical queries).  Vertex (i, j) sits at cell coordinates (i + dx, j + dy), as terrain_query_warped
// reads them.
__device__ float tw_cell(const ShfTerrain& T, const int16_t* __restrict__ H, int i0, int j0, const float* o, const float* d,
                         float s_min, float s_max, float* n) {
  const int rows = T.rows, cols = T.cols;
  const uint8_t* Wb = reinterpret_cast<const uint8_t*>(H + (size_t)rows * cols);
  const float hs = T.hscale, vs = T.vscale, bd = T.border, ih = 1.0f / hs;
  const int wc = Wb[(size_t)i0 * cols + j0];
  const int ilo = ((wc >> 4) & 1) && i0 > 0 ? i0 - 1 : i0, ihi = ((wc >> 5) & 1) && i0 < rows - 2 ? i0 + 1 : i0;
  const int jlo = ((wc >> 6) & 1) && j0 > 0 ? j0 - 1 : j0, jhi = ((wc >> 7) & 1) && j0 < cols - 2 ? j0 + 1 : j0;
  const float x0 = (float)i0 * hs - bd, y0 = (float)j0 * hs - bd;
  float best = INFINITY;
  for (int i = ilo; i <= ihi; i++)
    for (int j = jlo; j <= jhi; j++) {
      float P[4][3];
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
          const size_t idx = (size_t)(i + a) * cols + (j + b);
          const int wv = Wb[idx];
          P[2 * a + b][0] = (float)(i + a + (wv & 3) - 1) * hs - bd;
          P[2 * a + b][1] = (float)(j + b + ((wv >> 2) & 3) - 1) * hs - bd;
          P[2 * a + b][2] = (float)H[idx] * vs;
        }
      tw_triangle(o, d, P[0], P[3], P[1], s_min, s_max, x0, y0, ih, &best, n);
      tw_triangle(o, d, P[0], P[2], P[3], s_min, s_max, x0, y0, ih, &best, n);
    }
  return best;
}

// nearest front-facing height-field surface with s in [near, s_max]; the walk covers [near, s_max] clipped to the field's
// bounding box, cell by cell in ray order (the first cell with a hit holds the nearest one: a front face is entered at most
// once per cell, the two triangles being a graph over it).  TW: the warped trimesh instead -- the same clip (shifted
// vertices stay inside the grid, zmin / zmax bound z) and the same walk; a cell takes the nearest of the hits inside its
// square (tw_cell), so the first cell with a hit again holds the nearest one.
template <bool TW>
__device__ float hit_heightfield(const ShfTerrain& T, const int16_t* __restrict__ H, float zmin, float zmax, const float* o,
                                 const float* d, float s_min, float s_max, float* n) {
  const int rows = T.rows, cols = T.cols;
  const float hs = T.hscale, vs = T.vscale, bd = T.border;
  const float lo[3] = {-bd, -bd, zmin}, hi[3] = {(float)(rows - 1) * hs - bd, (float)(cols - 1) * hs - bd, zmax};
  float s0 = s_min, s1 = s_max;
  for (int k = 0; k < 3; k++) {
    if (d[k] == 0.0f) {
      if (o[k] < lo[k] || o[k] > hi[k]) return INFINITY;
      continue;
    }
    const float inv = 1.0f / d[k];
    const float t1 = (lo[k] - o[k]) * inv, t2 = (hi[k] - o[k]) * inv;
    s0 = fmaxf(s0, fminf(t1, t2));
    s1 = fminf(s1, fmaxf(t1, t2));
  }
  if (!(s0 <= s1)) return INFINITY;
  const float ih = 1.0f / hs;
  const float fx = (o[0] + s0 * d[0] + bd) * ih, fy = (o[1] + s0 * d[1] + bd) * ih;
  int i = (int)fminf(fmaxf(floorf(fx), 0.0f), (float)(rows - 2));
  int j = (int)fminf(fmaxf(floorf(fy), 0.0f), (float)(cols - 2));
  const int si = d[0] > 0.0f ? 1 : -1, sj = d[1] > 0.0f ? 1 : -1;
  const float tdx = d[0] != 0.0f ? hs / fabsf(d[0]) : INFINITY, tdy = d[1] != 0.0f ? hs / fabsf(d[1]) : INFINITY;
  float sx = d[0] != 0.0f ? ((float)(i + (si > 0 ? 1 : 0)) * hs - bd - o[0]) / d[0] : INFINITY;
  float sy = d[1] != 0.0f ? ((float)(j + (sj > 0 ? 1 : 0)) * hs - bd - o[1]) / d[1] : INFINITY;
  const float eps = 1e-5f;
  for (int it = 0; it < rows + cols; it++) {
    if constexpr (TW) {
      const float bt = tw_cell(T, H, i, j, o, d, s_min, s_max, n);
      if (bt < INFINITY) return bt;
    } else {
      const int16_t* r0 = H + (size_t)i * cols + j;
      const int16_t* r1 = r0 + cols;
      const float x0 = (float)i * hs - bd, y0 = (float)j * hs - bd, x1 = x0 + hs, y1 = y0 + hs;
      const float v00[3] = {x0, y0, (float)r0[0] * vs}, v10[3] = {x1, y0, (float)r1[0] * vs};
      const float v01[3] = {x0, y1, (float)r0[1] * vs}, v11[3] = {x1, y1, (float)r1[1] * vs};
      float best = INFINITY, s, nn[3];
      // lower triangle (u + v <= 1) and upper one (u + v >= 1), (u, v) the hit's position in the cell
      if (hf_triangle(o, d, v00, v10, v01, &s, nn) && s >= s_min && s <= s_max) {
        const float u = (o[0] + s * d[0] - x0) * ih, v = (o[1] + s * d[1] - y0) * ih;
        if (u >= -eps && v >= -eps && u + v <= 1.0f + eps && s < best) { best = s; n[0] = nn[0]; n[1] = nn[1]; n[2] = nn[2]; }
      }
      if (hf_triangle(o, d, v11, v01, v10, &s, nn) && s >= s_min && s <= s_max) {
        const float u = (o[0] + s * d[0] - x0) * ih, v = (o[1] + s * d[1] - y0) * ih;
        if (u <= 1.0f + eps && v <= 1.0f + eps && u + v >= 1.0f - eps && s < best) { best = s; n[0] = nn[0]; n[1] = nn[1]; n[2] = nn[2]; }
      }
      if (best < INFINITY) return best;
    }
    if (fminf(sx, sy) > s1) break;
    if (sx < sy) {
      i += si; sx += tdx;
      if (i < 0 || i > rows - 2) break;
    } else {
      j += sj; sy += tdy;
      if (j < 0 || j > cols - 2) break;
    }
  }
  return INFINITY;
}

__device__ __forceinline__ uint32_t shade_u8(float c, float lam) {
  const float v = fminf(fmaxf(c * lam, 0.0f), 1.0f);
  return (uint32_t)floorf(v * 255.0f + 0.5f);
}

}  // namespace

// TW: the terrain is a warped trimesh (hsamp: samples followed by one byte per vertex).  The two forms are two kernels
// (k_render_cameras, k_render_cameras_tw below); the host launches the TW one only when ShfTerrain.warped, so height fields
// and planes keep their code and registers.  FLOW: the optical-flow form (header comment), again kernels of their own names
// (k_render_cameras_flow, k_render_cameras_tw_flow): everything it adds sits behind if constexpr, so the plain kernels keep
// their code.
template <bool TW, bool FLOW>
__device__ __forceinline__ void render_cameras(const ShfRenderScene* __restrict__ scene, const ShfTerrain& T,
                                               const int16_t* __restrict__ hsamp, const ShfCamera& cam, int tiles_x, int tiles,
                                               const float* __restrict__ body_state, const float* __restrict__ cam_pose,
                                               const int32_t* __restrict__ seg_ids, const float* __restrict__ colors,
                                               float* __restrict__ depth, int32_t* __restrict__ seg_out, uint32_t* __restrict__ rgba,
                                               const float* __restrict__ prev_body_pose = nullptr,
                                               const float* __restrict__ prev_cam_pose = nullptr,
                                               const int32_t* __restrict__ prev_valid = nullptr, float2* __restrict__ flow = nullptr,
                                               uint32_t* __restrict__ flow_i16 = nullptr) {
  __shared__ float S[SHF_RENDER_MAX_SHAPES * RT_SW];
  __shared__ int SI[SHF_RENDER_MAX_SHAPES * 3];   // kind, poly, segmentation id
  // FLOW: per shape, the body's motion since the previous render about the camera origin, and whether its pose changed bits
  __shared__ float SM[FLOW ? SHF_RENDER_MAX_SHAPES * RT_MW : 1];
  __shared__ int SMV[FLOW ? SHF_RENDER_MAX_SHAPES : 1];
  const int env = blockIdx.x / tiles, tile = blockIdx.x - env * tiles;
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int lid = threadIdx.x, wave = lid >> 6, lane = lid & 63;
  const int W = cam.width, Hh = cam.height;
  // (the scene is device data: its counts are clamped to the LDS tables here, not trusted)
  const int ns = min(max(scene->nshapes, 0), SHF_RENDER_MAX_SHAPES), B = max(scene->num_bodies, 1);

  // camera basis: fwd = local +x, up = local +z, right = -(local +y)
  const float* cp = cam_pose + (size_t)env * 7;
  float Rc[9];
  {
    const float q[4] = {cp[3], cp[4], cp[5], cp[6]};
    quat_mat(q, Rc);
  }
  const float o[3] = {cp[0], cp[1], cp[2]};
  const float fwd[3] = {Rc[0], Rc[3], Rc[6]}, right[3] = {-Rc[1], -Rc[4], -Rc[7]}, up[3] = {Rc[2], Rc[5], Rc[8]};
  const float t = tanf(0.5f * cam.horizontal_fov * 0.017453292519943295f);
  const float ty_scale = t * (float)Hh / (float)W;

  if (lid < ns) {
    const ShfRenderShape& sh = scene->shape[lid];
    const size_t row = (size_t)env * B + min(max(sh.body, 0), B - 1);
    const float* bsr = body_state + row * 13;
    float Rb[9];
    {
      const float q[4] = {bsr[3], bsr[4], bsr[5], bsr[6]};
      quat_mat(q, Rb);
    }
    float* s = S + lid * RT_SW;
    for (int r = 0; r < 3; r++) {
      s[r] = bsr[r] + Rb[3 * r] * sh.pos[0] + Rb[3 * r + 1] * sh.pos[1] + Rb[3 * r + 2] * sh.pos[2];
      for (int c = 0; c < 3; c++)
        s[3 + 3 * r + c] = Rb[3 * r] * sh.rot[c] + Rb[3 * r + 1] * sh.rot[3 + c] + Rb[3 * r + 2] * sh.rot[6 + c];
      s[12 + r] = sh.param[r];
      s[16 + r] = colors[row * 3 + r];
    }
    s[15] = sh.radius;
    SI[lid * 3] = sh.kind;
    SI[lid * 3 + 1] = sh.poly;
    SI[lid * 3 + 2] = seg_ids[row];
    if constexpr (FLOW) {
      const float* pb = prev_body_pose + row * 7;
      bool mv = false;
      for (int k = 0; k < 7; k++) mv = mv || __float_as_uint(pb[k]) != __float_as_uint(bsr[k]);
      float* m = SM + lid * RT_MW;
      if (mv) {
        float Rp[9];
        {
          const float q[4] = {pb[3], pb[4], pb[5], pb[6]};
          quat_mat(q, Rp);
        }
        const float rel[3] = {bsr[0] - o[0], bsr[1] - o[1], bsr[2] - o[2]};
        for (int r = 0; r < 3; r++) {
          for (int c = 0; c < 3; c++) m[3 * r + c] = Rp[3 * r] * Rb[3 * c] + Rp[3 * r + 1] * Rb[3 * c + 1] + Rp[3 * r + 2] * Rb[3 * c + 2];
          m[9 + r] = (pb[r] - o[r]) - (m[3 * r] * rel[0] + m[3 * r + 1] * rel[1] + m[3 * r + 2] * rel[2]);
        }
      } else {
        for (int k = 0; k < RT_MW; k++) m[k] = (k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f;
      }
      SMV[lid] = mv ? 1 : 0;
    }
  }
  __syncthreads();

  // this wave's strip: columns [c0, c0 + 16), rows [r0, r0 + 4)
  const int c0 = tx * RT_TILE, r0 = ty * RT_TILE + wave * 4;
  const int col = c0 + (lane & 15), rowp = r0 + (lane >> 4);
  const float iW = 1.0f / (float)W, iH = 1.0f / (float)Hh;

  // per-wave cull: the cone around the strip's central ray that holds its four corner rays, against each shape's
  // bounding sphere and the [near, far] depth range (lane k tests shape k)
  uint64_t cand;
  {
    const float xa = 2.0f * (float)c0 * iW - 1.0f, xb = 2.0f * (float)(c0 + RT_TILE) * iW - 1.0f;
    const float ya = 1.0f - 2.0f * (float)r0 * iH, yb = 1.0f - 2.0f * (float)(r0 + 4) * iH;
    float ax[3];
    for (int k = 0; k < 3; k++) ax[k] = fwd[k] + right[k] * (0.5f * (xa + xb) * t) + up[k] * (0.5f * (ya + yb) * ty_scale);
    const float ian = 1.0f / sqrtf(dot3(ax, ax));
    for (int k = 0; k < 3; k++) ax[k] *= ian;
    float cmin = 1.0f;
    for (int e = 0; e < 4; e++) {
      const float xx = (e & 1) ? xb : xa, yy = (e & 2) ? yb : ya;
      float dd[3];
      for (int k = 0; k < 3; k++) dd[k] = fwd[k] + right[k] * (xx * t) + up[k] * (yy * ty_scale);
      cmin = fminf(cmin, dot3(dd, ax) / sqrtf(dot3(dd, dd)));
    }
    const float half = acosf(fminf(fmaxf(cmin, -1.0f), 1.0f));
    bool hit = false;
    if (lane < ns) {
      const float* s = S + lane * RT_SW;
      const float v[3] = {s[0] - o[0], s[1] - o[1], s[2] - o[2]};
      const float r = s[15], dist2 = dot3(v, v), dv = dot3(v, fwd);
      if (dv - r <= cam.far_plane && dv + r >= cam.near_plane) {
        if (dist2 <= r * r) {
          hit = true;
        } else {
          const float dist = sqrtf(dist2);
          const float ang = acosf(fminf(fmaxf(dot3(v, ax) / dist, -1.0f), 1.0f));
          hit = ang <= half + asinf(fminf(r / dist, 1.0f)) + 1e-3f;
        }
      }
    }
    cand = __ballot(hit);
  }

  const float px = 2.0f * ((float)col + 0.5f) * iW - 1.0f, py = 1.0f - 2.0f * ((float)rowp + 0.5f) * iH;
  float d[3];
  for (int k = 0; k < 3; k++) d[k] = fwd[k] + right[k] * (px * t) + up[k] * (py * ty_scale);
  const float nearp = cam.near_plane, farp = cam.far_plane;

  float best = INFINITY, nw[3] = {0.0f, 0.0f, 1.0f};
  int best_i = -1;
  while (cand) {
    const int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(cand));
    cand &= cand - 1;
    const float* s = S + i * RT_SW;
    const float rel[3] = {o[0] - s[0], o[1] - s[1], o[2] - s[2]};
    float ol[3], dl[3];
    for (int k = 0; k < 3; k++) {     // into the shape frame: R^T (.)
      ol[k] = s[3 + k] * rel[0] + s[6 + k] * rel[1] + s[9 + k] * rel[2];
      dl[k] = s[3 + k] * d[0] + s[6 + k] * d[1] + s[9 + k] * d[2];
    }
    const int kind = SI[i * 3];
    float nl[3] = {0.0f, 0.0f, 1.0f}, sh;
    if (kind == SHF_RENDER_BOX) {
      const float h[3] = {s[12], s[13], s[14]};
      sh = hit_box(ol, dl, h, nl);
    } else if (kind == SHF_RENDER_SPHERE) {
      sh = hit_sphere(ol, dl, s[12], nl);
    } else if (kind == SHF_RENDER_CAPSULE) {
      sh = hit_capsule(ol, dl, s[12], s[13], nl);
    } else {
      const int p = __builtin_amdgcn_readfirstlane(min(max(SI[i * 3 + 1], 0), SHF_RENDER_MAX_POLYS - 1));
      sh = hit_poly(&scene->poly[p], ol, dl, nl);
    }
    if (sh >= nearp && sh <= farp && sh < best) {
      best = sh;
      best_i = i;
      for (int k = 0; k < 3; k++) nw[k] = s[3 + 3 * k] * nl[0] + s[4 + 3 * k] * nl[1] + s[5 + 3 * k] * nl[2];
    }
  }

  int sid = 0;
  float base[3] = {0.0f, 0.0f, 0.0f};
  bool ground_hit = false;
  if (scene->ground) {
    const float lim = fminf(best, farp);
    float nn[3], sg = INFINITY;
    if (T.rows == 0) {
      if (d[2] < 0.0f) {
        const float s = -o[2] / d[2];
        if (s >= nearp && s <= lim) { sg = s; nn[0] = 0.0f; nn[1] = 0.0f; nn[2] = 1.0f; }
      }
    } else {
      sg = hit_heightfield<TW>(T, hsamp, scene->hf_zmin, scene->hf_zmax, o, d, nearp, lim, nn);
    }
    if (sg < best) {
      best = sg;
      ground_hit = true;
      nw[0] = nn[0]; nw[1] = nn[1]; nw[2] = nn[2];
      base[0] = scene->ground_color[0]; base[1] = scene->ground_color[1]; base[2] = scene->ground_color[2];
    }
  }
  if (!ground_hit && best_i >= 0) {
    const float* s = S + best_i * RT_SW;
    base[0] = s[16]; base[1] = s[17]; base[2] = s[18];
    sid = SI[best_i * 3 + 2];
  }

  if (col >= W || rowp >= Hh) return;
  const size_t px_i = ((size_t)env * Hh + rowp) * W + col;
  const bool any = best < INFINITY;
  if (depth) {
    const float dv = any ? best : INFINITY;
    depth[px_i] = cam.depth_negative ? -dv : dv;
  }
  if (seg_out) seg_out[px_i] = sid;
  if (rgba) {
    uint32_t pix;
    if (any) {
      const float il = 1.0f / sqrtf(dot3(nw, nw));
      const float nl = (nw[0] * SHF_RENDER_LIGHT_X + nw[1] * SHF_RENDER_LIGHT_Y + nw[2] * SHF_RENDER_LIGHT_Z) * il;
      const float lam = SHF_RENDER_AMBIENT + SHF_RENDER_DIFFUSE * fmaxf(nl, 0.0f);
      pix = shade_u8(base[0], lam) | (shade_u8(base[1], lam) << 8) | (shade_u8(base[2], lam) << 16) | (255u << 24);
    } else {
      pix = (uint32_t)SHF_RENDER_BG_R | ((uint32_t)SHF_RENDER_BG_G << 8) | ((uint32_t)SHF_RENDER_BG_B << 16) | (255u << 24);
    }
    rgba[px_i] = pix;
  }
  if constexpr (FLOW) {
    float fu = 0.0f, fv = 0.0f;
    if (any && prev_valid[env] != 0) {
      // the previous camera: its basis as the current one's above, its origin relative to the current one's
      const float* pc = prev_cam_pose + (size_t)env * 7;
      bool moved = false;
      for (int k = 0; k < 7; k++) moved = moved || __float_as_uint(pc[k]) != __float_as_uint(cp[k]);
      // X' - o: the hit point about the camera origin, carried by its body's motion (the terrain: as it is)
      float v[3] = {best * d[0], best * d[1], best * d[2]};
      if (!ground_hit && best_i >= 0) {
        const float* m = SM + best_i * RT_MW;
        moved = moved || SMV[best_i] != 0;
        const float x[3] = {v[0], v[1], v[2]};
        for (int k = 0; k < 3; k++) v[k] = (m[3 * k] * x[0] + m[3 * k + 1] * x[1] + m[3 * k + 2] * x[2]) + m[9 + k];
      }
      if (moved) {
        float Rp[9];
        {
          const float q[4] = {pc[3], pc[4], pc[5], pc[6]};
          quat_mat(q, Rp);
        }
        for (int k = 0; k < 3; k++) v[k] -= pc[k] - o[k];
        const float fwdp[3] = {Rp[0], Rp[3], Rp[6]}, rightp[3] = {-Rp[1], -Rp[4], -Rp[7]}, upp[3] = {Rp[2], Rp[5], Rp[8]};
        const float zp = dot3(fwdp, v);
        const float xp = dot3(rightp, v) / (zp * t), yp = dot3(upp, v) / (zp * ty_scale);
        const float cpx = (xp + 1.0f) * (0.5f * (float)W) - 0.5f, rpx = (1.0f - yp) * (0.5f * (float)Hh) - 0.5f;
        const float u = (float)col - cpx, w = (float)rowp - rpx;
        if (zp > 0.0f && isfinite(u) && isfinite(w)) { fu = u; fv = w; }
      }
    }
    if (flow) flow[px_i] = make_float2(fu, fv);
    if (flow_i16) {
      // Isaac Gym's encoding: u x 32768 is exact, one correctly rounded division, round half to even, saturate
      const float qu = fminf(fmaxf(rintf((fu * 32768.0f) / (float)W), -32768.0f), 32767.0f);
      const float qv = fminf(fmaxf(rintf((fv * 32768.0f) / (float)Hh), -32768.0f), 32767.0f);
      flow_i16[px_i] = ((uint32_t)(int)qu & 0xffffu) | ((uint32_t)(int)qv << 16);
    }
  }
}

#define RT_KERNEL_ARGS                                                                                                          \
  const ShfRenderScene *__restrict__ scene, ShfTerrain T, const int16_t *__restrict__ hsamp, ShfCamera cam, int tiles_x,        \
      int tiles, const float *__restrict__ body_state, const float *__restrict__ cam_pose, const int32_t *__restrict__ seg_ids, \
      const float *__restrict__ colors, float *__restrict__ depth, int32_t *__restrict__ seg_out, uint32_t *__restrict__ rgba

__global__ void __launch_bounds__(RT_THREADS) k_render_cameras(RT_KERNEL_ARGS) {
  render_cameras<false, false>(scene, T, hsamp, cam, tiles_x, tiles, body_state, cam_pose, seg_ids, colors, depth, seg_out, rgba);
}
__global__ void __launch_bounds__(RT_THREADS) k_render_cameras_tw(RT_KERNEL_ARGS) {
  render_cameras<true, false>(scene, T, hsamp, cam, tiles_x, tiles, body_state, cam_pose, seg_ids, colors, depth, seg_out, rgba);
}

#define RT_FLOW_KERNEL_ARGS                                                                                          \
  RT_KERNEL_ARGS, const float *__restrict__ prev_body_pose, const float *__restrict__ prev_cam_pose,                 \
      const int32_t *__restrict__ prev_valid, float2 *__restrict__ flow, uint32_t *__restrict__ flow_i16

__global__ void __launch_bounds__(RT_THREADS) k_render_cameras_flow(RT_FLOW_KERNEL_ARGS) {
  render_cameras<false, true>(scene, T, hsamp, cam, tiles_x, tiles, body_state, cam_pose, seg_ids, colors, depth, seg_out, rgba,
                              prev_body_pose, prev_cam_pose, prev_valid, flow, flow_i16);
}
__global__ void __launch_bounds__(RT_THREADS) k_render_cameras_tw_flow(RT_FLOW_KERNEL_ARGS) {
  render_cameras<true, true>(scene, T, hsamp, cam, tiles_x, tiles, body_state, cam_pose, seg_ids, colors, depth, seg_out, rgba,
                             prev_body_pose, prev_cam_pose, prev_valid, flow, flow_i16);
}

// The argument checks both entries share (fn: the entry's name, the prefix of its error strings).  Returns 0 with *tiles_x /
// *tiles set, or the error code.
static int render_check(const char* fn, const ShfRenderScene* scene_dev, const ShfTerrain* terrain, const int16_t* height_samples_dev,
                        const ShfCamera* camera, int32_t num_envs, int* tiles_x, int* tiles) {
  const std::string f(fn);
  if (!scene_dev || !terrain || !camera) return shf_set_error(f + ": null scene, terrain or camera");
  const ShfCamera& c = *camera;
  if (c.width <= 0 || c.height <= 0 || c.width > 16384 || c.height > 16384)
    return shf_set_error(f + ": width and height must be in 1..16384");
  if (!(c.horizontal_fov > 0.0f && c.horizontal_fov < 180.0f))
    return shf_set_error(f + ": horizontal_fov must be in (0, 180) degrees");
  if (!(c.near_plane > 0.0f && c.far_plane > c.near_plane)) return shf_set_error(f + ": need 0 < near_plane < far_plane");
  if (terrain->warped && terrain->rows == 0) return shf_set_error(f + ": a warped (trimesh) terrain needs height samples");
  if (terrain->rows != 0 && (terrain->rows < 2 || terrain->cols < 2 || !height_samples_dev))
    return shf_set_error(f + ": a height field needs at least 2 x 2 samples on the device");
  if (num_envs < 0) return shf_set_error(f + ": num_envs < 0");
  *tiles_x = (c.width + RT_TILE - 1) / RT_TILE;
  *tiles = *tiles_x * ((c.height + RT_TILE - 1) / RT_TILE);
  return 0;
}

extern "C" int shf_render_cameras(const ShfRenderScene* scene_dev, const ShfTerrain* terrain, const int16_t* height_samples_dev,
                                  const ShfCamera* camera, int32_t num_envs, const float* body_state, const float* cam_pose,
                                  const int32_t* seg_ids, const float* colors, float* depth_or_null, int32_t* seg_or_null,
                                  uint8_t* rgba_or_null, void* stream) {
  int tiles_x, tiles;
  if (const int rc = render_check("shf_render_cameras", scene_dev, terrain, height_samples_dev, camera, num_envs, &tiles_x, &tiles)) return rc;
  if (num_envs == 0 || (!depth_or_null && !seg_or_null && !rgba_or_null)) return 0;
  if (!body_state || !cam_pose || !seg_ids || !colors) return shf_set_error("shf_render_cameras: null input tensor");
  if ((int64_t)tiles * num_envs > 0x7fffffffLL) return shf_set_error("shf_render_cameras: too many envs x tiles for one launch");
  hipLaunchKernelGGL(terrain->warped ? k_render_cameras_tw : k_render_cameras, dim3((unsigned)(tiles * num_envs)),
                     dim3(RT_THREADS), 0, (hipStream_t)stream, scene_dev, *terrain, height_samples_dev, *camera, tiles_x, tiles,
                     body_state, cam_pose, seg_ids, colors, depth_or_null, seg_or_null, reinterpret_cast<uint32_t*>(rgba_or_null));
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_render_cameras: launch failed");
}

// The flow form: shf_render_cameras' arguments in their places, then the previous render's poses and the flow images.
extern "C" int shf_render_cameras_flow(const ShfRenderScene* scene_dev, const ShfTerrain* terrain, const int16_t* height_samples_dev,
                                       const ShfCamera* camera, int32_t num_envs, const float* body_state, const float* cam_pose,
                                       const int32_t* seg_ids, const float* colors, float* depth_or_null, int32_t* seg_or_null,
                                       uint8_t* rgba_or_null, const float* prev_body_pose, const float* prev_cam_pose,
                                       const int32_t* prev_valid, float* flow_or_null, int16_t* flow_i16_or_null, void* stream) {
  if (!flow_or_null && !flow_i16_or_null)
    return shf_render_cameras(scene_dev, terrain, height_samples_dev, camera, num_envs, body_state, cam_pose, seg_ids, colors,
                              depth_or_null, seg_or_null, rgba_or_null, stream);
  int tiles_x, tiles;
  if (const int rc = render_check("shf_render_cameras_flow", scene_dev, terrain, height_samples_dev, camera, num_envs, &tiles_x, &tiles)) return rc;
  if (num_envs == 0) return 0;
  if (!body_state || !cam_pose || !seg_ids || !colors) return shf_set_error("shf_render_cameras_flow: null input tensor");
  if (!prev_body_pose || !prev_cam_pose || !prev_valid)
    return shf_set_error("shf_render_cameras_flow: null prev_body_pose, prev_cam_pose or prev_valid");
  if (((uintptr_t)flow_or_null & 7u) != 0 || ((uintptr_t)flow_i16_or_null & 3u) != 0)
    return shf_set_error("shf_render_cameras_flow: flow must be 8-byte aligned and flow_i16 4-byte aligned");
  if ((int64_t)tiles * num_envs > 0x7fffffffLL) return shf_set_error("shf_render_cameras_flow: too many envs x tiles for one launch");
  hipLaunchKernelGGL(terrain->warped ? k_render_cameras_tw_flow : k_render_cameras_flow, dim3((unsigned)(tiles * num_envs)),
                     dim3(RT_THREADS), 0, (hipStream_t)stream, scene_dev, *terrain, height_samples_dev, *camera, tiles_x, tiles,
                     body_state, cam_pose, seg_ids, colors, depth_or_null, seg_or_null, reinterpret_cast<uint32_t*>(rgba_or_null),
                     prev_body_pose, prev_cam_pose, prev_valid, reinterpret_cast<float2*>(flow_or_null),
                     reinterpret_cast<uint32_t*>(flow_i16_or_null));
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_render_cameras_flow: launch failed");
}

// ---- world view (shf_render_world; the headless viewer of shifu_amd/viewer.py) -------------------------------------------
// One camera that sees many envs.  One 256-thread workgroup per (view, 16 x 16 tile), a wave per 16 x 4 strip, as above; the
// drawn envs are walked in passes of RW_CHUNK / nshapes envs, one thread per (env of the pass, shape): the thread builds its
// shape's world centre (body pose, then the env's offset) and tests the bounding sphere against the TILE's cone and
// [near, far].  The survivors are compacted IN ORDER -- a ballot, a popcount prefix, the four wave totals through LDS; no
// atomics, which would make the order depend on timing -- into a candidate list in LDS (RW_LIST records: the 20 floats of the
// per-env kernels' table, then kind, poly, segmentation id and env id).  When the next pass could overflow the list, and
// after the last pass, it is flushed: every wave casts its pixels against the list (64 records at a time through its own strip cull, then the
// wave-uniform candidate loop of the per-env kernels) and keeps the nearest hit under a strict <, and the list restarts.
// Records are cast in (list position, shape) order whatever the flushes, so on equal depth the earlier one wins and the
// images do not depend on where the flushes fall.  The terrain is cast last, up to the nearest shape, and wins only where
// it is strictly nearer: k_render_cameras' rule.  env_radius > 0 adds a pass in front: one thread per env tests the env's
// sphere against the tile's cone, and only the surviving envs (compacted in order into EL) reach the shape passes.
#define RW_LIST SHF_RENDER_WORLD_LIST
#define RW_CHUNK SHF_RENDER_WORLD_CHUNK
#define RW_REC 24     // dwords per record: RT_SW floats, then kind, poly, segmentation id, env id
static_assert(RW_CHUNK == RT_THREADS, "one thread per (env, shape) pair of a pass");
static_assert(RW_LIST >= RW_CHUNK, "a pass must fit the empty list");

namespace {

// the cone about the central ray of pixel columns [ca, cb) x rows [ra, rb) that holds their four corner rays
__device__ __forceinline__ void rw_cone(const float* fwd, const float* right, const float* up, float xa, float xb, float ya,
                                        float yb, float t, float ty_scale, float* ax, float* half) {
  for (int k = 0; k < 3; k++) ax[k] = fwd[k] + right[k] * (0.5f * (xa + xb) * t) + up[k] * (0.5f * (ya + yb) * ty_scale);
  const float ian = 1.0f / sqrtf(dot3(ax, ax));
  for (int k = 0; k < 3; k++) ax[k] *= ian;
  float cmin = 1.0f;
  for (int e = 0; e < 4; e++) {
    const float xx = (e & 1) ? xb : xa, yy = (e & 2) ? yb : ya;
    float dd[3];
    for (int k = 0; k < 3; k++) dd[k] = fwd[k] + right[k] * (xx * t) + up[k] * (yy * ty_scale);
    cmin = fminf(cmin, dot3(dd, ax) / sqrtf(dot3(dd, dd)));
  }
  *half = acosf(fminf(fmaxf(cmin, -1.0f), 1.0f));
}

// does the sphere of radius r about v (relative to the camera origin) reach into the cone and the depth range?
__device__ __forceinline__ bool rw_sphere_in_cone(const float* v, float r, const float* ax, float half, const float* fwd,
                                                  float nearp, float farp) {
  const float dist2 = dot3(v, v), dv = dot3(v, fwd);
  if (!(dv - r <= farp && dv + r >= nearp)) return false;
  if (dist2 <= r * r) return true;
  const float dist = sqrtf(dist2);
  const float ang = acosf(fminf(fmaxf(dot3(v, ax) / dist, -1.0f), 1.0f));
  return ang <= half + asinf(fminf(r / dist, 1.0f)) + 1e-3f;
}

struct RwHit {
  float best, nw[3], col[3];
  int sid, env;
};

// a flush: this wave's pixels against records [0, count) of the list, in order
__device__ __forceinline__ void rw_cast(const float* L, int count, const ShfRenderScene* __restrict__ scene, const float* o,
                                        const float* d, const float* fwd, const float* sax, float shalf, float nearp, float farp,
                                        int lane, RwHit& h) {
  for (int b0 = 0; b0 < count; b0 += 64) {
    bool in = false;
    if (b0 + lane < count) {
      const float* s = L + (b0 + lane) * RW_REC;
      const float v[3] = {s[0] - o[0], s[1] - o[1], s[2] - o[2]};
      in = rw_sphere_in_cone(v, s[15], sax, shalf, fwd, nearp, farp);
    }
    uint64_t cand = __ballot(in);
    while (cand) {
      const int i = b0 + __builtin_amdgcn_readfirstlane(__builtin_ctzll(cand));
      cand &= cand - 1;
      const float* s = L + i * RW_REC;
      const float rel[3] = {o[0] - s[0], o[1] - s[1], o[2] - s[2]};
      float ol[3], dl[3];
      for (int k = 0; k < 3; k++) {     // into the shape frame: R^T (.)
        ol[k] = s[3 + k] * rel[0] + s[6 + k] * rel[1] + s[9 + k] * rel[2];
        dl[k] = s[3 + k] * d[0] + s[6 + k] * d[1] + s[9 + k] * d[2];
      }
      const int kind = __float_as_int(s[20]);
      float nl[3] = {0.0f, 0.0f, 1.0f}, sh;
      if (kind == SHF_RENDER_BOX) {
        const float hh[3] = {s[12], s[13], s[14]};
        sh = hit_box(ol, dl, hh, nl);
      } else if (kind == SHF_RENDER_SPHERE) {
        sh = hit_sphere(ol, dl, s[12], nl);
      } else if (kind == SHF_RENDER_CAPSULE) {
        sh = hit_capsule(ol, dl, s[12], s[13], nl);
      } else {
        const int p = __builtin_amdgcn_readfirstlane(min(max(__float_as_int(s[21]), 0), SHF_RENDER_MAX_POLYS - 1));
        sh = hit_poly(&scene->poly[p], ol, dl, nl);
      }
      if (sh >= nearp && sh <= farp && sh < h.best) {
        h.best = sh;
        for (int k = 0; k < 3; k++) h.nw[k] = s[3 + 3 * k] * nl[0] + s[4 + 3 * k] * nl[1] + s[5 + 3 * k] * nl[2];
        h.col[0] = s[16]; h.col[1] = s[17]; h.col[2] = s[18];
        h.sid = __float_as_int(s[22]);
        h.env = __float_as_int(s[23]);
      }
    }
  }
}

// exclusive prefix of `keep` over the workgroup in thread order, and the total: a ballot and a popcount per wave, the wave
// totals through WT (the caller alternates between two WT rows, so one barrier per call is enough)
__device__ __forceinline__ int rw_prefix(bool keep, int* WT, int wave, int lane, int* total) {
  const uint64_t m = __ballot(keep);
  if (lane == 0) WT[wave] = __popcll(m);
  __syncthreads();
  int pre = __popcll(m & ((1ull << lane) - 1ull)), tot = 0;
  for (int w = 0; w < RT_THREADS / 64; w++) {
    const int c = WT[w];
    if (w < wave) pre += c;
    tot += c;
  }
  *total = tot;
  return pre;
}

}  // namespace

template <bool TW>
__device__ __forceinline__ void render_world(const ShfRenderScene* __restrict__ scene, const ShfTerrain& T,
                                             const int16_t* __restrict__ hsamp, const ShfCamera& cam, int tiles_x, int tiles,
                                             const float* __restrict__ view_pose, int num_envs, int num_drawn,
                                             const int32_t* __restrict__ env_ids, const float* __restrict__ env_offset,
                                             float env_radius, const float* __restrict__ body_state,
                                             const int32_t* __restrict__ seg_ids, const float* __restrict__ colors,
                                             float* __restrict__ depth, int32_t* __restrict__ seg_out, uint32_t* __restrict__ rgba,
                                             int32_t* __restrict__ env_out) {
  __shared__ float L[RW_LIST * RW_REC];
  __shared__ int EL[RT_THREADS];                  // env pre-cull: the surviving list positions of a block of RT_THREADS
  __shared__ int WT[2][RT_THREADS / 64];
  const int view = blockIdx.x / tiles, tile = blockIdx.x - view * tiles;
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int lid = threadIdx.x, wave = lid >> 6, lane = lid & 63;
  const int W = cam.width, Hh = cam.height;
  // (device data, not trusted: the counts are clamped, and so is every env id below)
  const int ns = min(max(scene->nshapes, 0), SHF_RENDER_MAX_SHAPES), B = max(scene->num_bodies, 1);

  const float* cp = view_pose + (size_t)view * 7;
  float Rc[9];
  {
    const float q[4] = {cp[3], cp[4], cp[5], cp[6]};
    quat_mat(q, Rc);
  }
  const float o[3] = {cp[0], cp[1], cp[2]};
  const float fwd[3] = {Rc[0], Rc[3], Rc[6]}, right[3] = {-Rc[1], -Rc[4], -Rc[7]}, up[3] = {Rc[2], Rc[5], Rc[8]};
  const float t = tanf(0.5f * cam.horizontal_fov * 0.017453292519943295f);
  const float ty_scale = t * (float)Hh / (float)W;
  const float nearp = cam.near_plane, farp = cam.far_plane;

  const int c0 = tx * RT_TILE, r0 = ty * RT_TILE + wave * 4;
  const int col = c0 + (lane & 15), rowp = r0 + (lane >> 4);
  const float iW = 1.0f / (float)W, iH = 1.0f / (float)Hh;
  const float xa = 2.0f * (float)c0 * iW - 1.0f, xb = 2.0f * (float)(c0 + RT_TILE) * iW - 1.0f;
  float tax[3], thalf, sax[3], shalf;     // the tile's cone (what enters the list) and this wave's strip's (its own cull)
  rw_cone(fwd, right, up, xa, xb, 1.0f - 2.0f * (float)(ty * RT_TILE) * iH, 1.0f - 2.0f * (float)(ty * RT_TILE + RT_TILE) * iH, t,
          ty_scale, tax, &thalf);
  rw_cone(fwd, right, up, xa, xb, 1.0f - 2.0f * (float)r0 * iH, 1.0f - 2.0f * (float)(r0 + 4) * iH, t, ty_scale, sax, &shalf);

  const float px = 2.0f * ((float)col + 0.5f) * iW - 1.0f, py = 1.0f - 2.0f * ((float)rowp + 0.5f) * iH;
  float d[3];
  for (int k = 0; k < 3; k++) d[k] = fwd[k] + right[k] * (px * t) + up[k] * (py * ty_scale);

  RwHit h;
  h.best = INFINITY;
  h.nw[0] = 0.0f; h.nw[1] = 0.0f; h.nw[2] = 1.0f;
  h.col[0] = h.col[1] = h.col[2] = 0.0f;
  h.sid = 0;
  h.env = -1;

  if (ns > 0) {
    const int ec = RW_CHUNK / ns;                   // envs per pass (>= 4: ns <= 64)
    const int je = lid / ns, si = lid - je * ns;    // this thread's env of the pass and its shape
    const bool cull = env_radius > 0.0f;
    int count = 0, par = 0;
    for (int base = 0; base < num_drawn; base += RT_THREADS) {
      int nel = min(RT_THREADS, num_drawn - base);
      if (cull) {
        bool keep = false;
        if (lid < nel) {
          const int j = base + lid;
          const int env = min(max(env_ids ? env_ids[j] : j, 0), num_envs - 1);
          const float* bsr = body_state + (size_t)env * B * 13;
          float v[3];
          for (int k = 0; k < 3; k++) v[k] = (bsr[k] + (env_offset ? env_offset[(size_t)j * 3 + k] : 0.0f)) - o[k];
          keep = rw_sphere_in_cone(v, env_radius, tax, thalf, fwd, nearp, farp);
        }
        const int pre = rw_prefix(keep, WT[par], wave, lane, &nel);
        par ^= 1;
        if (keep) EL[pre] = base + lid;
        __syncthreads();
      }
      // (at least one pass per block, possibly an empty one: the flush below is the only one, and the last pass takes it)
      int e0 = 0;
      do {
        const int ne = max(min(ec, nel - e0), 0);
        bool keep = false;
        int env = 0;
        size_t row = 0;
        float c[3] = {0.0f, 0.0f, 0.0f}, Rb[9];
        if (je < ne) {
          const int j = cull ? EL[e0 + je] : base + e0 + je;
          env = min(max(env_ids ? env_ids[j] : j, 0), num_envs - 1);
          const ShfRenderShape& sh = scene->shape[si];
          row = (size_t)env * B + min(max(sh.body, 0), B - 1);
          const float* bsr = body_state + row * 13;
          {
            const float q[4] = {bsr[3], bsr[4], bsr[5], bsr[6]};
            quat_mat(q, Rb);
          }
          for (int r = 0; r < 3; r++)
            c[r] = (bsr[r] + Rb[3 * r] * sh.pos[0] + Rb[3 * r + 1] * sh.pos[1] + Rb[3 * r + 2] * sh.pos[2]) +
                   (env_offset ? env_offset[(size_t)j * 3 + r] : 0.0f);
          const float v[3] = {c[0] - o[0], c[1] - o[1], c[2] - o[2]};
          keep = rw_sphere_in_cone(v, sh.radius, tax, thalf, fwd, nearp, farp);
        }
        int total;
        const int pre = rw_prefix(keep, WT[par], wave, lane, &total);
        par ^= 1;
        if (keep) {
          const ShfRenderShape& sh = scene->shape[si];
          float* s = L + (count + pre) * RW_REC;
          for (int r = 0; r < 3; r++) {
            s[r] = c[r];
            for (int cc = 0; cc < 3; cc++)
              s[3 + 3 * r + cc] = Rb[3 * r] * sh.rot[cc] + Rb[3 * r + 1] * sh.rot[3 + cc] + Rb[3 * r + 2] * sh.rot[6 + cc];
            s[12 + r] = sh.param[r];
            s[16 + r] = colors[row * 3 + r];
          }
          s[15] = sh.radius;
          s[19] = 0.0f;
          s[20] = __int_as_float(sh.kind);
          s[21] = __int_as_float(sh.poly);
          s[22] = __int_as_float(seg_ids[row]);
          s[23] = __int_as_float(env);
        }
        count += total;
        e0 += ec;
        // flush: after the last pass, and when the next pass could overflow the list
        if ((e0 >= nel && base + RT_THREADS >= num_drawn) || count + ec * ns > RW_LIST) {
          __syncthreads();
          rw_cast(L, count, scene, o, d, fwd, sax, shalf, nearp, farp, lane, h);
          __syncthreads();
          count = 0;
        }
      } while (e0 < nel);
    }
  }

  float best = h.best;
  bool ground_hit = false;
  if (scene->ground) {
    const float lim = fminf(best, farp);
    float nn[3], sg = INFINITY;
    if (T.rows == 0) {
      if (d[2] < 0.0f) {
        const float s = -o[2] / d[2];
        if (s >= nearp && s <= lim) { sg = s; nn[0] = 0.0f; nn[1] = 0.0f; nn[2] = 1.0f; }
      }
    } else {
      sg = hit_heightfield<TW>(T, hsamp, scene->hf_zmin, scene->hf_zmax, o, d, nearp, lim, nn);
    }
    if (sg < best) {
      best = sg;
      ground_hit = true;
      h.nw[0] = nn[0]; h.nw[1] = nn[1]; h.nw[2] = nn[2];
      h.col[0] = scene->ground_color[0]; h.col[1] = scene->ground_color[1]; h.col[2] = scene->ground_color[2];
    }
  }

  if (col >= W || rowp >= Hh) return;
  const size_t px_i = ((size_t)view * Hh + rowp) * W + col;
  const bool any = best < INFINITY;
  if (depth) {
    const float dv = any ? best : INFINITY;
    depth[px_i] = cam.depth_negative ? -dv : dv;
  }
  if (seg_out) seg_out[px_i] = ground_hit ? 0 : h.sid;
  if (env_out) env_out[px_i] = ground_hit ? -1 : h.env;
  if (rgba) {
    uint32_t pix;
    if (any) {
      const float il = 1.0f / sqrtf(dot3(h.nw, h.nw));
      const float nl = (h.nw[0] * SHF_RENDER_LIGHT_X + h.nw[1] * SHF_RENDER_LIGHT_Y + h.nw[2] * SHF_RENDER_LIGHT_Z) * il;
      const float lam = SHF_RENDER_AMBIENT + SHF_RENDER_DIFFUSE * fmaxf(nl, 0.0f);
      pix = shade_u8(h.col[0], lam) | (shade_u8(h.col[1], lam) << 8) | (shade_u8(h.col[2], lam) << 16) | (255u << 24);
    } else {
      pix = (uint32_t)SHF_RENDER_BG_R | ((uint32_t)SHF_RENDER_BG_G << 8) | ((uint32_t)SHF_RENDER_BG_B << 16) | (255u << 24);
    }
    rgba[px_i] = pix;
  }
}

#define RW_KERNEL_ARGS                                                                                                       \
  const ShfRenderScene *__restrict__ scene, ShfTerrain T, const int16_t *__restrict__ hsamp, ShfCamera cam, int tiles_x,     \
      int tiles, const float *__restrict__ view_pose, int num_envs, int num_drawn, const int32_t *__restrict__ env_ids,      \
      const float *__restrict__ env_offset, float env_radius, const float *__restrict__ body_state,                         \
      const int32_t *__restrict__ seg_ids, const float *__restrict__ colors, float *__restrict__ depth,                      \
      int32_t *__restrict__ seg_out, uint32_t *__restrict__ rgba, int32_t *__restrict__ env_out

__global__ void __launch_bounds__(RT_THREADS) k_render_world(RW_KERNEL_ARGS) {
  render_world<false>(scene, T, hsamp, cam, tiles_x, tiles, view_pose, num_envs, num_drawn, env_ids, env_offset, env_radius,
                      body_state, seg_ids, colors, depth, seg_out, rgba, env_out);
}
__global__ void __launch_bounds__(RT_THREADS) k_render_world_tw(RW_KERNEL_ARGS) {
  render_world<true>(scene, T, hsamp, cam, tiles_x, tiles, view_pose, num_envs, num_drawn, env_ids, env_offset, env_radius,
                     body_state, seg_ids, colors, depth, seg_out, rgba, env_out);
}

extern "C" int shf_render_world(const ShfRenderScene* scene_dev, const ShfTerrain* terrain, const int16_t* height_samples_dev,
                                const ShfCamera* camera, int32_t num_views, const float* view_pose, int32_t num_envs,
                                int32_t num_drawn, const int32_t* env_ids_or_null, const float* env_offset_or_null, float env_radius,
                                const float* body_state, const int32_t* seg_ids, const float* colors, float* depth_or_null,
                                int32_t* seg_or_null, uint8_t* rgba_or_null, int32_t* env_or_null, void* stream) {
  int tiles_x, tiles;
  if (const int rc = render_check("shf_render_world", scene_dev, terrain, height_samples_dev, camera, num_envs, &tiles_x, &tiles)) return rc;
  if (num_views < 1 || num_envs < 1 || num_drawn < 1)
    return shf_set_error("shf_render_world: num_views, num_envs and num_drawn must be at least 1");
  if (!body_state || !view_pose || !seg_ids || !colors) return shf_set_error("shf_render_world: null input tensor");
  if (((uintptr_t)rgba_or_null & 3u) != 0) return shf_set_error("shf_render_world: rgba must be 4-byte aligned");
  if ((int64_t)tiles * num_views > 0x7fffffffLL) return shf_set_error("shf_render_world: too many views x tiles for one launch");
  if (!depth_or_null && !seg_or_null && !rgba_or_null && !env_or_null) return 0;
  hipLaunchKernelGGL(terrain->warped ? k_render_world_tw : k_render_world, dim3((unsigned)(tiles * num_views)), dim3(RT_THREADS),
                     0, (hipStream_t)stream, scene_dev, *terrain, height_samples_dev, *camera, tiles_x, tiles, view_pose, num_envs,
                     num_drawn, env_ids_or_null, env_offset_or_null, env_radius, body_state, seg_ids, colors, depth_or_null,
                     seg_or_null, reinterpret_cast<uint32_t*>(rgba_or_null), env_or_null);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_render_world: launch failed");
}

// ---- ray caster (shf_raycast; lidar, height scanners, point clouds -- shifu_amd/raycast.py) ---------------------------------
// Arbitrary rays, the same for every env, from a sensor pose per env: ray r of env e starts at p_e + R o_r and runs along
// unit(R d_r), R the sensor's rotation as `align` takes it.  The ray parameter is the Euclidean range, so [min_range,
// max_range] are ranges where the cameras' [near, far] are view depths; otherwise the cameras' hit rule and tie rules.
// One 256-thread workgroup per (env, chunk of 256 rays), one ray per lane; the env's shape world poses are staged once per
// workgroup into LDS (one thread per shape, no colors).  There is no strip and so no cone: the loop over the unmasked shapes
// is wave-uniform, every lane tests its own ray -- the closest approach of the segment [min_range, min(best, max_range)] to
// the shape's bounding sphere -- and a ballot skips the shape for the wave when no lane can hit it; the lanes that passed
// run the closed form.  The test is conservative (RC_SLACK), so a lane's result is what it is with the cull off
// (shf_raycast_debug_cull), and it never depends on the other lanes.  The checker is tests/raycast_ref.py.
#define RC_SW 16   // floats per shape in LDS: c[3] R[9] param[3] radius

namespace {

// Can the ray (o, unit d) meet the sphere (c, r) at a range in [t0, t1]?  The closest point of that segment to the centre,
// against r plus a slack far above the float32 error of either this test or the closed forms (both ~1e-7 of the distances
// involved): 1e-3 r + 1e-4 m + 1e-5 of the range of closest approach.  A NaN fails, as it fails the closed forms' range test.
__device__ __forceinline__ bool rc_may_hit(const float* o, const float* d, const float* c, float r, float t0, float t1) {
  const float v[3] = {c[0] - o[0], c[1] - o[1], c[2] - o[2]};
  const float tc = fminf(fmaxf(dot3(v, d), t0), t1);
  const float w[3] = {v[0] - tc * d[0], v[1] - tc * d[1], v[2] - tc * d[2]};
  const float re = r * 1.001f + 1e-4f + 1e-5f * (tc + r);
  return dot3(w, w) <= re * re;
}

}  // namespace

template <bool TW>
__device__ __forceinline__ void raycast(const ShfRenderScene* __restrict__ scene, const ShfTerrain& T,
                                        const int16_t* __restrict__ hsamp, int num_rays, int chunks,
                                        const float* __restrict__ ray_origin, const float* __restrict__ ray_dir,
                                        const float* __restrict__ body_state, const float* __restrict__ sensor_pose, int align,
                                        float min_range, float max_range, uint64_t shape_mask, const int32_t* __restrict__ seg_ids,
                                        float* __restrict__ dist, float* __restrict__ points, float* __restrict__ normal,
                                        int32_t* __restrict__ seg_out, int32_t* __restrict__ body_out, int cull) {
  __shared__ float S[SHF_RENDER_MAX_SHAPES * RC_SW];
  __shared__ int SI[SHF_RENDER_MAX_SHAPES * 4];   // kind, poly, segmentation id, body row within the env
  const int env = blockIdx.x / chunks, chunk = blockIdx.x - env * chunks;
  const int lid = threadIdx.x;
  const int ray = chunk * RT_THREADS + lid;
  const bool active = ray < num_rays;
  // (the scene is device data: its counts are clamped to the LDS tables here, not trusted)
  const int ns = min(max(scene->nshapes, 0), SHF_RENDER_MAX_SHAPES), B = max(scene->num_bodies, 1);

  if (lid < ns) {
    const ShfRenderShape& sh = scene->shape[lid];
    const int brow = min(max(sh.body, 0), B - 1);
    const size_t row = (size_t)env * B + brow;
    const float* bsr = body_state + row * 13;
    float Rb[9];
    {
      const float q[4] = {bsr[3], bsr[4], bsr[5], bsr[6]};
      quat_mat(q, Rb);
    }
    float* s = S + lid * RC_SW;
    for (int r = 0; r < 3; r++) {
      s[r] = bsr[r] + Rb[3 * r] * sh.pos[0] + Rb[3 * r + 1] * sh.pos[1] + Rb[3 * r + 2] * sh.pos[2];
      for (int c = 0; c < 3; c++)
        s[3 + 3 * r + c] = Rb[3 * r] * sh.rot[c] + Rb[3 * r + 1] * sh.rot[3 + c] + Rb[3 * r + 2] * sh.rot[6 + c];
      s[12 + r] = sh.param[r];
    }
    s[15] = sh.radius;
    SI[lid * 4] = sh.kind;
    SI[lid * 4 + 1] = sh.poly;
    SI[lid * 4 + 2] = seg_ids ? seg_ids[row] : 0;
    SI[lid * 4 + 3] = brow;
  }

  // the sensor's rotation as `align` takes it: all of it, its yaw about world z only, or none
  const float* sp = sensor_pose + (size_t)env * 7;
  float Rs[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  if (align != SHF_RAY_ALIGN_WORLD) {
    const float q[4] = {sp[3], sp[4], sp[5], sp[6]};
    quat_mat(q, Rs);
    if (align == SHF_RAY_ALIGN_YAW) {
      // Rz(atan2(R10, R00)) by its cosine and sine (R00, R10) / |(R00, R10)|; the sensor's x axis vertical: no yaw
      const float h = sqrtf(Rs[0] * Rs[0] + Rs[3] * Rs[3]);
      const float cy = h > 0.0f ? Rs[0] / h : 1.0f, sy = h > 0.0f ? Rs[3] / h : 0.0f;
      Rs[0] = cy;   Rs[1] = -sy;  Rs[2] = 0.0f;
      Rs[3] = sy;   Rs[4] = cy;   Rs[5] = 0.0f;
      Rs[6] = 0.0f; Rs[7] = 0.0f; Rs[8] = 1.0f;
    }
  }
  float o[3] = {sp[0], sp[1], sp[2]}, d[3] = {1.0f, 0.0f, 0.0f};
  bool valid = false;   // a ray of this pattern with a usable direction; the others vote "no" and cast nothing
  if (active) {
    const float* ro = ray_origin + (size_t)ray * 3;
    const float* rd = ray_dir + (size_t)ray * 3;
    const float a[3] = {ro[0], ro[1], ro[2]}, b[3] = {rd[0], rd[1], rd[2]};
    float dw[3];
    for (int k = 0; k < 3; k++) {
      o[k] += Rs[3 * k] * a[0] + Rs[3 * k + 1] * a[1] + Rs[3 * k + 2] * a[2];
      dw[k] = Rs[3 * k] * b[0] + Rs[3 * k + 1] * b[1] + Rs[3 * k + 2] * b[2];
    }
    const float l2 = dot3(dw, dw);
    if (l2 > 0.0f && l2 < INFINITY) {      // (a NaN fails both)
      const float il = 1.0f / sqrtf(l2);
      for (int k = 0; k < 3; k++) d[k] = dw[k] * il;
      valid = true;
    }
  }
  __syncthreads();

  float best = INFINITY, nw[3] = {0.0f, 0.0f, 0.0f};
  int best_i = -1;
  for (int i = 0; i < ns; i++) {
    if (!((shape_mask >> i) & 1ull)) continue;
    const float* s = S + i * RC_SW;
    const bool may = valid && (!cull || rc_may_hit(o, d, s, s[15], min_range, fminf(best, max_range)));
    if (!__ballot(may)) continue;
    if (!may) continue;
    const float rel[3] = {o[0] - s[0], o[1] - s[1], o[2] - s[2]};
    float ol[3], dl[3];
    for (int k = 0; k < 3; k++) {     // into the shape frame: R^T (.)
      ol[k] = s[3 + k] * rel[0] + s[6 + k] * rel[1] + s[9 + k] * rel[2];
      dl[k] = s[3 + k] * d[0] + s[6 + k] * d[1] + s[9 + k] * d[2];
    }
    const int kind = SI[i * 4];
    float nl[3] = {0.0f, 0.0f, 1.0f}, sh;
    if (kind == SHF_RENDER_BOX) {
      const float h[3] = {s[12], s[13], s[14]};
      sh = hit_box(ol, dl, h, nl);
    } else if (kind == SHF_RENDER_SPHERE) {
      sh = hit_sphere(ol, dl, s[12], nl);
    } else if (kind == SHF_RENDER_CAPSULE) {
      sh = hit_capsule(ol, dl, s[12], s[13], nl);
    } else {
      const int p = __builtin_amdgcn_readfirstlane(min(max(SI[i * 4 + 1], 0), SHF_RENDER_MAX_POLYS - 1));
      sh = hit_poly(&scene->poly[p], ol, dl, nl);
    }
    if (sh >= min_range && sh <= max_range && sh < best) {
      best = sh;
      best_i = i;
      for (int k = 0; k < 3; k++) nw[k] = s[3 + 3 * k] * nl[0] + s[4 + 3 * k] * nl[1] + s[5 + 3 * k] * nl[2];
    }
  }

  if (valid && scene->ground) {
    const float lim = fminf(best, max_range);
    float nn[3], sg = INFINITY;
    if (T.rows == 0) {
      if (d[2] < 0.0f) {
        const float s = -o[2] / d[2];
        if (s >= min_range && s <= lim) { sg = s; nn[0] = 0.0f; nn[1] = 0.0f; nn[2] = 1.0f; }
      }
    } else {
      sg = hit_heightfield<TW>(T, hsamp, scene->hf_zmin, scene->hf_zmax, o, d, min_range, lim, nn);
    }
    if (sg < best) {      // the terrain wins only where it is strictly nearer
      best = sg;
      best_i = -1;
      nw[0] = nn[0]; nw[1] = nn[1]; nw[2] = nn[2];
    }
  }

  if (!active) return;
  const size_t ri = (size_t)env * num_rays + ray;
  const bool any = best < INFINITY;
  if (dist) dist[ri] = any ? best : INFINITY;
  if (points) {
    // the hit, or the ray's end at max_range (finite); a ray without a direction: its origin
    const float s = any ? best : (valid ? max_range : 0.0f);
    float* p = points + ri * 3;
    p[0] = o[0] + s * d[0]; p[1] = o[1] + s * d[1]; p[2] = o[2] + s * d[2];
  }
  if (normal) {
    float* n = normal + ri * 3;
    if (any) {
      const float il = 1.0f / sqrtf(dot3(nw, nw));
      n[0] = nw[0] * il; n[1] = nw[1] * il; n[2] = nw[2] * il;
    } else {
      n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
    }
  }
  if (seg_out) seg_out[ri] = any && best_i >= 0 ? SI[best_i * 4 + 2] : 0;
  if (body_out) body_out[ri] = !any ? -2 : best_i >= 0 ? SI[best_i * 4 + 3] : -1;
}

#define RC_KERNEL_ARGS                                                                                                        \
  const ShfRenderScene *__restrict__ scene, ShfTerrain T, const int16_t *__restrict__ hsamp, int num_rays, int chunks,        \
      const float *__restrict__ ray_origin, const float *__restrict__ ray_dir, const float *__restrict__ body_state,          \
      const float *__restrict__ sensor_pose, int align, float min_range, float max_range, uint64_t shape_mask,                \
      const int32_t *__restrict__ seg_ids, float *__restrict__ dist, float *__restrict__ points, float *__restrict__ normal,  \
      int32_t *__restrict__ seg_out, int32_t *__restrict__ body_out, int cull

__global__ void __launch_bounds__(RT_THREADS) k_raycast(RC_KERNEL_ARGS) {
  raycast<false>(scene, T, hsamp, num_rays, chunks, ray_origin, ray_dir, body_state, sensor_pose, align, min_range, max_range,
                 shape_mask, seg_ids, dist, points, normal, seg_out, body_out, cull);
}
__global__ void __launch_bounds__(RT_THREADS) k_raycast_tw(RC_KERNEL_ARGS) {
  raycast<true>(scene, T, hsamp, num_rays, chunks, ray_origin, ray_dir, body_state, sensor_pose, align, min_range, max_range,
                shape_mask, seg_ids, dist, points, normal, seg_out, body_out, cull);
}

// the per-ray cull of the launches that follow (a host-side debug switch: the tests assert that it changes no bit)
static int g_raycast_cull = 1;

extern "C" int shf_raycast_debug_cull(int32_t enable) {
  const int was = g_raycast_cull;
  g_raycast_cull = enable ? 1 : 0;
  return was;
}

extern "C" int shf_raycast(const ShfRenderScene* scene_dev, const ShfTerrain* terrain, const int16_t* height_samples_dev,
                           int32_t num_envs, int32_t num_rays, const float* ray_origin, const float* ray_dir,
                           const float* body_state, const float* sensor_pose, int32_t align, float min_range, float max_range,
                           uint64_t shape_mask, const int32_t* seg_ids, float* dist_or_null, float* points_or_null,
                           float* normal_or_null, int32_t* seg_or_null, int32_t* body_or_null, void* stream) {
  if (!scene_dev || !terrain) return shf_set_error("shf_raycast: null scene or terrain");
  if (num_envs < 1 || num_rays < 1) return shf_set_error("shf_raycast: num_envs and num_rays must be at least 1");
  if (!ray_origin || !ray_dir || !body_state || !sensor_pose) return shf_set_error("shf_raycast: null input tensor");
  if (!dist_or_null && !points_or_null && !normal_or_null && !seg_or_null && !body_or_null)
    return shf_set_error("shf_raycast: every output is null");
  if (align < SHF_RAY_ALIGN_BASE || align > SHF_RAY_ALIGN_WORLD) return shf_set_error("shf_raycast: align must be SHF_RAY_ALIGN_BASE, _YAW or _WORLD");
  if (!(min_range >= 0.0f && min_range <= max_range) || !(max_range < INFINITY))
    return shf_set_error("shf_raycast: need 0 <= min_range <= max_range, max_range finite");
  if (seg_or_null && !seg_ids) return shf_set_error("shf_raycast: a seg output needs seg_ids");
  if (terrain->warped && terrain->rows == 0) return shf_set_error("shf_raycast: a warped (trimesh) terrain needs height samples");
  if (terrain->rows != 0 && (terrain->rows < 2 || terrain->cols < 2 || !height_samples_dev))
    return shf_set_error("shf_raycast: a height field needs at least 2 x 2 samples on the device");
  const int64_t chunks = ((int64_t)num_rays + RT_THREADS - 1) / RT_THREADS;
  if (chunks * num_envs > 0x7fffffffLL) return shf_set_error("shf_raycast: too many envs x ray chunks for one launch");
  hipLaunchKernelGGL(terrain->warped ? k_raycast_tw : k_raycast, dim3((unsigned)(chunks * num_envs)), dim3(RT_THREADS), 0,
                     (hipStream_t)stream, scene_dev, *terrain, height_samples_dev, num_rays, (int)chunks, ray_origin, ray_dir,
                     body_state, sensor_pose, align, min_range, max_range, shape_mask, seg_ids, dist_or_null, points_or_null,
                     normal_or_null, seg_or_null, body_or_null, g_raycast_cull);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_raycast: launch failed");
}

// The point behind every pixel of a rendered depth image: X = o + s d, d the camera convention's pixel ray (its component
// along the view axis is 1, so s is the view depth) and s = |depth| -- either sign convention of ShfCamera.depth_negative; a
// depth that is not finite (nothing hit): s = far_plane.  One pixel per lane, a 12-byte store each.
__global__ void __launch_bounds__(RT_THREADS) k_camera_points(ShfCamera cam, size_t total, const float* __restrict__ depth,
                                                              const float* __restrict__ cam_pose, int world_frame,
                                                              float* __restrict__ points) {
  const size_t i = (size_t)blockIdx.x * RT_THREADS + threadIdx.x;
  if (i >= total) return;
  const int W = cam.width, Hh = cam.height;
  const size_t hw = (size_t)W * Hh;
  const size_t env = i / hw;
  const int pix = (int)(i - env * hw);
  const int rowp = pix / W, col = pix - rowp * W;
  const float t = tanf(0.5f * cam.horizontal_fov * 0.017453292519943295f);
  const float ty_scale = t * (float)Hh / (float)W;
  const float iW = 1.0f / (float)W, iH = 1.0f / (float)Hh;
  const float px = 2.0f * ((float)col + 0.5f) * iW - 1.0f, py = 1.0f - 2.0f * ((float)rowp + 0.5f) * iH;
  const float dv = fabsf(depth[i]);
  const float s = dv < INFINITY ? dv : cam.far_plane;     // (a NaN fails the comparison too)
  float* p = points + i * 3;
  if (world_frame) {
    const float* cp = cam_pose + env * 7;
    float Rc[9];
    {
      const float q[4] = {cp[3], cp[4], cp[5], cp[6]};
      quat_mat(q, Rc);
    }
    const float fwd[3] = {Rc[0], Rc[3], Rc[6]}, right[3] = {-Rc[1], -Rc[4], -Rc[7]}, up[3] = {Rc[2], Rc[5], Rc[8]};
    for (int k = 0; k < 3; k++) p[k] = cp[k] + s * (fwd[k] + right[k] * (px * t) + up[k] * (py * ty_scale));
  } else {
    // the camera's own axes: +x the view axis, +y to the left (right = -y), +z up
    p[0] = s; p[1] = -(s * (px * t)); p[2] = s * (py * ty_scale);
  }
}

extern "C" int shf_camera_points(const ShfCamera* camera, int32_t num_envs, const float* depth, const float* cam_pose,
                                 int32_t world_frame, float* points, void* stream) {
  if (!camera) return shf_set_error("shf_camera_points: null camera");
  const ShfCamera& c = *camera;
  if (c.width <= 0 || c.height <= 0 || c.width > 16384 || c.height > 16384)
    return shf_set_error("shf_camera_points: width and height must be in 1..16384");
  if (!(c.horizontal_fov > 0.0f && c.horizontal_fov < 180.0f))
    return shf_set_error("shf_camera_points: horizontal_fov must be in (0, 180) degrees");
  if (!(c.far_plane > 0.0f && c.far_plane < INFINITY)) return shf_set_error("shf_camera_points: far_plane must be positive and finite");
  if (num_envs < 1) return shf_set_error("shf_camera_points: num_envs must be at least 1");
  if (!depth || !points || (world_frame && !cam_pose)) return shf_set_error("shf_camera_points: null depth, points or cam_pose");
  const size_t total = (size_t)num_envs * c.width * c.height;
  const size_t blocks = (total + RT_THREADS - 1) / RT_THREADS;
  if (blocks > 0x7fffffffULL) return shf_set_error("shf_camera_points: too many pixels for one launch");
  hipLaunchKernelGGL(k_camera_points, dim3((unsigned)blocks), dim3(RT_THREADS), 0, (hipStream_t)stream, c, total, depth, cam_pose,
                     world_frame, points);
  return hipGetLastError() == hipSuccess ? 0 : shf_set_error("shf_camera_points: launch failed");
}
