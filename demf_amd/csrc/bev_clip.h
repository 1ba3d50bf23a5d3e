// Exact rotated-footprint clip of two depth boxes and the 3-D IoU built on it: shared by the evaluation
// (csrc/eval3d.hip) and the rotated NMS of the test-time augmentation merge (csrc/tta.hip).
// Boxes are upstream's bottom-centre form (x, y, z_bottom, dx, dy, dz, yaw).  All arithmetic is fp32
// (build: -ffp-contract=off); tests/test_gpu_eval.py pins it.
#pragma once
#include <hip/hip_runtime.h>

namespace demf {

constexpr int kClipVerts = 8;        // polygon buffer of the footprint clip (see clip_half_plane)

// Keep the half-plane  sgn * p[axis] <= h  of the convex polygon (in, n) -> (out, return count).
// Inclusive test, so touching and collinear edges keep their vertices; a crossing edge gets the
// vertex on the clip line with the clip coordinate set exactly.  An exactly convex input gives at most
// n + 1 vertices (4 -> 8 over the four clips); a polygon made slightly non-convex by fp32 rounding could
// give more, so every write is capped at the buffer's kClipVerts = 8 and a surplus vertex of such a
// sliver is dropped (8 keeps both buffers in registers; 12 puts them in scratch).
template <int AXIS>
__device__ __forceinline__ int clip_half_plane(const float (*in)[2], int n, float (*out)[2], float sgn,
                                               float h) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const float* p = in[i];
    const float* q = in[i + 1 == n ? 0 : i + 1];
    const float dp = sgn * p[AXIS] - h, dq = sgn * q[AXIS] - h;
    const bool ip = dp <= 0.f, iq = dq <= 0.f;
    if (ip != iq && m < kClipVerts) {
      const float t = dp / (dp - dq);     // dp and dq have opposite signs: |dp - dq| > 0
      out[m][AXIS] = sgn * h;
      out[m][1 - AXIS] = p[1 - AXIS] + t * (q[1 - AXIS] - p[1 - AXIS]);
      ++m;
    }
    if (iq && m < kClipVerts) {
      out[m][0] = q[0];
      out[m][1] = q[1];
      ++m;
    }
  }
  return m;
}

// Area of footprint(a) ∩ footprint(b).  Frame: centred on box a, axes along a's local axes, where a is
// [-dx/2, dx/2] x [-dy/2, dy/2].  Local corner u of a box maps to the world as
// R(yaw) u + centre with R(t) u = (u.x cos t + u.y sin t, -u.x sin t + u.y cos t) (postprocess.hip
// box_extent_count_k, geometry.rotation_3d_in_axis_z); R is a rotation group, so b's corners in a's
// frame are R(yaw_b - yaw_a) u + R(-yaw_a) (centre_b - centre_a).  b's quad is clipped by a's four
// half-planes (at most 8 vertices for an exactly convex quad) and the shoelace sum gives the area.
__device__ __forceinline__ float bev_overlap(const float* a, const float* b) {
  const float ca = cosf(a[6]), sa = sinf(a[6]);
  const float tx = b[0] - a[0], ty = b[1] - a[1];
  const float cx = tx * ca - ty * sa, cy = tx * sa + ty * ca;     // R(-yaw_a) (centre_b - centre_a)
  const float th = b[6] - a[6];
  const float c = cosf(th), s = sinf(th);
  const float hbx = b[3] * 0.5f, hby = b[4] * 0.5f;
  float p0[kClipVerts][2], p1[kClipVerts][2];
  const float ux[4] = {-hbx, hbx, hbx, -hbx}, uy[4] = {-hby, -hby, hby, hby};   // counter-clockwise
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    p0[k][0] = (ux[k] * c + uy[k] * s) + cx;
    p0[k][1] = ((-ux[k]) * s + uy[k] * c) + cy;
  }
  const float hx = a[3] * 0.5f, hy = a[4] * 0.5f;
  int n = clip_half_plane<0>(p0, 4, p1, 1.f, hx);
  n = clip_half_plane<0>(p1, n, p0, -1.f, hx);
  n = clip_half_plane<1>(p0, n, p1, 1.f, hy);
  n = clip_half_plane<1>(p1, n, p0, -1.f, hy);
  float area2 = 0.f;
  for (int i = 0; i < n; ++i) {
    const float* p = p0[i];
    const float* q = p0[i + 1 == n ? 0 : i + 1];
    area2 += p[0] * q[1] - q[0] * p[1];
  }
  return fabsf(area2) * 0.5f;
}

// BaseInstance3DBoxes.overlaps(a, b, mode='iou') for depth boxes (bottom-centre form).
__device__ __forceinline__ float box3d_iou(const float* a, const float* b) {
  const float h = fmaxf(fminf(a[2] + a[5], b[2] + b[5]) - fmaxf(a[2], b[2]), 0.f);
  const float inter = bev_overlap(a, b) * h;
  const float va = a[3] * a[4] * a[5], vb = b[3] * b[4] * b[5];
  return inter / fmaxf(va + vb - inter, 1e-8f);
}

}  // namespace demf
