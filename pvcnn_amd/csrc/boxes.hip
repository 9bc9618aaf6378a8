// boxes.hip -- oriented-box overlaps of the Frustum-PVCNN (KITTI) metrics: the meter update, per-pair box IoU, the AP evaluation's
// rotated BEV overlaps (rotate_iou_gpu_eval) and their fused 3-D form (d3_box_overlap), and the --evaluate prediction table.
//
// Reference: meters/kitti/frustum.py decodes the boxes with torch, copies the corners to the host and clips them in Python
// (meters/kitti/utils.py: Sutherland-Hodgman + scipy ConvexHull, once per box); evaluate/kitti/utils/iou.py is a numba.cuda kernel;
// evaluate/kitti/utils/eval.py:58-103 follows it with a host loop; evaluate/kitti/frustum/eval.py:168-244 decodes on the device and
// fills the table in a numba loop.  All four reduce to one geometric question -- the area of the intersection of two convex quads
// in bird's-eye view -- answered here by ONE device function (quad_overlap), in fp64 on the fp32 corners.
//
// quad_overlap is the shoelace area of A n B taken edge by edge: the boundary of A n B is the part of A's boundary inside B plus the
// part of B's boundary inside A, so twice its area is the sum of cross(p, q) over those clipped segments (Cyrus-Beck: every edge is
// clipped to a parameter range by the four closed half-planes of the other quad).  Fixed trip counts, no vertex list: it lives in
// registers.  No division can be 0/0 (a parameter is taken only where the two end values have opposite signs), so no NaN comes out
// of finite corners.  An edge lying ON a line of the other quad counts once, and only when both run the same way (A's copy is
// kept, B's dropped): identical boxes give exactly their own shoelace area (IoU exactly 1), boxes that touch along an edge give 0.
// A quad of zero area intersects nothing, and a union of 0 gives IoU 0.
#include <algorithm>

#include "common.h"

namespace pvcnn {

constexpr int kBoxThreads = 256;
constexpr int kBoxTile = 64;              // boxes and query boxes per tile of the N x K launch: 4 rows of 64 lanes, 16 pairs per lane
constexpr int kBoxMaxClasses = 64;        // class table of MeterFrustumKitti (KITTI has 3)
constexpr int kWrapCap = 64;              // angle-wrap steps of update_predictions (|angle| < ~200 rad); the reference loops forever

struct Quad {
  double x[4], y[4];
};

__device__ __forceinline__ double cross2(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

// twice the signed (shoelace) area
__device__ __forceinline__ double quad_area2(const Quad &q) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += cross2(q.x[i], q.y[i], q.x[(i + 1) & 3], q.y[(i + 1) & 3]);
  return s;
}

// counter-clockwise vertex order (v0, v3, v2, v1 when the quad is clockwise); returns twice the (non-negative) area
__device__ __forceinline__ double quad_ccw(Quad &q) {
  const bool cw = quad_area2(q) < 0.0;
  const double x1 = q.x[1], y1 = q.y[1];
  q.x[1] = cw ? q.x[3] : x1;
  q.y[1] = cw ? q.y[3] : y1;
  q.x[3] = cw ? x1 : q.x[3];
  q.y[3] = cw ? y1 : q.y[3];
  return quad_area2(q);
}

// twice the area contributed by the edges of P inside Q (both counter-clockwise); from_a: P is A (keeps same-direction
// collinear edges)
__device__ __forceinline__ double clipped_edges2(const Quad &P, const Quad &Q, bool from_a) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double px0 = P.x[i], py0 = P.y[i], px1 = P.x[(i + 1) & 3], py1 = P.y[(i + 1) & 3];
    double lo = 0.0, hi = 1.0;
    bool keep = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double ex = Q.x[(j + 1) & 3] - Q.x[j], ey = Q.y[(j + 1) & 3] - Q.y[j];
      const double f0 = cross2(ex, ey, px0 - Q.x[j], py0 - Q.y[j]);   // >= 0: inside (left of the edge)
      const double f1 = cross2(ex, ey, px1 - Q.x[j], py1 - Q.y[j]);
      if (f0 == 0.0 && f1 == 0.0) {
        keep = keep && from_a && (ex * (px1 - px0) + ey * (py1 - py0) > 0.0);
      } else if (f0 < 0.0 && f1 < 0.0) {
        keep = false;
      } else if (f0 < 0.0) {
        lo = fmax(lo, f0 / (f0 - f1));                                  // entering
      } else if (f1 < 0.0) {
        hi = fmin(hi, f0 / (f0 - f1));                                  // leaving
      }
    }
    if (keep && lo < hi) {
      // (1 - t) p0 + t p1 is exact at t = 0 and t = 1: an unclipped edge contributes exactly its shoelace term
      const double ax = (1.0 - lo) * px0 + lo * px1, ay = (1.0 - lo) * py0 + lo * py1;
      const double bx = (1.0 - hi) * px0 + hi * px1, by = (1.0 - hi) * py0 + hi * py1;
      s += cross2(ax, ay, bx, by);
    }
  }
  return s;
}

// Intersection area of two convex quads given by their corners in either orientation; area_a / area_b get their areas.
// Coordinates are taken relative to A's first corner (exact for fp32 inputs).
__device__ __forceinline__ double quad_overlap(const float (&ax)[4], const float (&ay)[4], const float (&bx)[4], const float (&by)[4],
                                               double &area_a, double &area_b) {
  const double ox = ax[0], oy = ay[0];
  Quad A, B;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    A.x[i] = (double)ax[i] - ox;
    A.y[i] = (double)ay[i] - oy;
    B.x[i] = (double)bx[i] - ox;
    B.y[i] = (double)by[i] - oy;
  }
  const double a2 = quad_ccw(A), b2 = quad_ccw(B);
  area_a = 0.5 * a2;
  area_b = 0.5 * b2;
  if (!(a2 > 0.0) || !(b2 > 0.0)) return 0.0;
  const double inter = 0.5 * (clipped_edges2(A, B, true) + clipped_edges2(B, A, false));
  return fmin(fmax(inter, 0.0), fmin(area_a, area_b));
}

__device__ __forceinline__ double safe_ratio(double num, double den) { return den > 0.0 ? num / den : 0.0; }

// ---- box IoU on (3, 8) corner sets (meters/kitti/utils.get_box_iou_3d) ------------------------------------------------------------
// BEV: the upper face's (x, z) of corners 3, 2, 1, 0; height overlap from the y of corners 0 (top) and 4 (bottom).  A box's volume
// is its BEV area times |y0 - y4| (the reference multiplies three corner distances: the same for a box; this form makes identical
// boxes give exactly 1).
struct BoxCorners {
  float x[4], z[4];                       // corners 3, 2, 1, 0
  float top, bottom;                      // y of corners 0 and 4
};

__device__ __forceinline__ void box_iou_3d(const BoxCorners &p, const BoxCorners &t, double &iou_3d, double &iou_2d) {
  double area_p, area_t;
  const double inter = quad_overlap(p.x, p.z, t.x, t.z, area_p, area_t);
  iou_2d = safe_ratio(inter, area_p + area_t - inter);
  const double y_max = fmin((double)p.top, (double)t.top), y_min = fmax((double)p.bottom, (double)t.bottom);
  const double inter_vol = inter * fmax(0.0, y_max - y_min);
  const double vol_p = area_p * fabs((double)p.top - (double)p.bottom), vol_t = area_t * fabs((double)t.top - (double)t.bottom);
  iou_3d = safe_ratio(inter_vol, vol_p + vol_t - inter_vol);
}

__device__ __forceinline__ BoxCorners load_corners(const float *__restrict__ c) {   // (3, 8) row-major
  BoxCorners b;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    b.x[i] = c[3 - i];
    b.z[i] = c[16 + 3 - i];
  }
  b.top = c[8 + 0];
  b.bottom = c[8 + 4];
  return b;
}

// ---- decode of the network's box outputs (meters/kitti/frustum.py:55-66, evaluate/kitti/frustum/eval.py:180-185) -----------------
// torch.argmax semantics: the first maximum; a NaN beats every number
__device__ __forceinline__ int box_argmax(const float *__restrict__ v, int n) {
  float best = v[0];
  int k = 0;
  for (int c = 1; c < n; ++c) {
    const float x = v[c];
    if (x > best || (x != x && best == best)) {
      best = x;
      k = c;
    }
  }
  return k;
}

// heading = bin_centers[id] + residual, size = templates[id] + residual (fp32, as torch adds them)
__device__ __forceinline__ float decode_heading(const float *__restrict__ bin_centers, int id, float residual) {
  return bin_centers[id] + residual;
}

// modules/frustum.get_box_corners_3d (with_flip=False) for the corners the IoU reads: R = roty(heading) applied to
// (+-l/2, +-h/2, +-w/2), x = c*lx + s*lz + cx, y = ly + cy, z = -s*lx + c*lz + cz in fp32
__device__ __forceinline__ BoxCorners make_corners(float cx, float cy, float cz, float heading, float l, float w, float h) {
  const float c = cosf(heading), s = sinf(heading);
  const float hl = l / 2.0f, hw = w / 2.0f, hh = h / 2.0f;
  // corners 3, 2, 1, 0 of the sign pattern x (1, 1, -1, -1), z (1, -1, -1, 1)
  const float lx[4] = {-hl, -hl, hl, hl}, lz[4] = {hw, -hw, -hw, hw};
  BoxCorners b;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    b.x[i] = (c * lx[i] + s * lz[i]) + cx;
    b.z[i] = (-s * lx[i] + c * lz[i]) + cz;
  }
  b.top = hh + cy;
  b.bottom = -hh + cy;
  return b;
}

struct BoxHeads {                         // network outputs of one batch (B rows)
  const float *center, *heading_scores, *heading_residuals, *size_scores, *size_residuals;
};

__device__ __forceinline__ void decode_prediction(const BoxHeads &o, int b, int NH, int NS, const float *__restrict__ bin_centers,
                                                  const float *__restrict__ templates, float &heading, float (&size)[3]) {
  const int hid = box_argmax(o.heading_scores + (long long)b * NH, NH);
  heading = decode_heading(bin_centers, hid, o.heading_residuals[(long long)b * NH + hid]);
  const int sid = box_argmax(o.size_scores + (long long)b * NS, NS);
#pragma unroll
  for (int c = 0; c < 3; ++c) size[c] = templates[sid * 3 + c] + o.size_residuals[((long long)b * NS + sid) * 3 + c];
}

// ---- MeterFrustumKitti.update, box metrics: one workgroup, fp64 sums reduced in a fixed order --------------------------------------
// sums (2) fp64 += [iou_2d, iou_3d]; counts (3 + 2K) int64 += [boxes, -, iou_3d >= 0.7, correct K | seen K]
struct MeterTargets {
  const float *center, *heading_residual, *size_residual;
  const long long *heading_bin_id, *size_template_id, *class_id;
};

__global__ __launch_bounds__(kBoxThreads) void frustum_meter_box_kernel(BoxHeads o, MeterTargets t, int B, int NH, int NS,
                                                                       const float *__restrict__ bin_centers,
                                                                       const float *__restrict__ templates,
                                                                       const long long *__restrict__ class_ids,
                                                                       const double *__restrict__ thresholds, int K, double *sums,
                                                                       long long *counts) {
  __shared__ double red[2][kBoxThreads];
  __shared__ unsigned hist[2 * kBoxMaxClasses + 1];
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * K + 1; i += kBoxThreads) hist[i] = 0u;
  __syncthreads();
  double s2 = 0.0, s3 = 0.0;
  for (int b = tid; b < B; b += kBoxThreads) {
    float heading, size[3];
    decode_prediction(o, b, NH, NS, bin_centers, templates, heading, size);
    const BoxCorners p = make_corners(o.center[3 * b], o.center[3 * b + 1], o.center[3 * b + 2], heading, size[0], size[1], size[2]);
    const long long hid = t.heading_bin_id[b], sid = t.size_template_id[b];
    double iou_3d = 0.0, iou_2d = 0.0;     // a target id outside its table: IoU 0 (the reference would raise)
    if (hid >= 0 && hid < NH && sid >= 0 && sid < NS) {
      const float heading_t = decode_heading(bin_centers, (int)hid, t.heading_residual[b]);
      float size_t_[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) size_t_[c] = templates[sid * 3 + c] + t.size_residual[3 * b + c];
      const BoxCorners q = make_corners(t.center[3 * b], t.center[3 * b + 1], t.center[3 * b + 2], heading_t, size_t_[0], size_t_[1],
                                        size_t_[2]);
      box_iou_3d(p, q, iou_3d, iou_2d);
    }
    s2 += iou_2d;
    s3 += iou_3d;
    if (iou_3d >= 0.7) atomicAdd(hist + 2 * K, 1u);
    const long long cls = t.class_id[b];
    for (int k = 0; k < K; ++k) {
      if (cls != class_ids[k]) continue;
      atomicAdd(hist + K + k, 1u);
      if (iou_3d >= thresholds[k]) atomicAdd(hist + k, 1u);
    }
  }
  red[0][tid] = s2;
  red[1][tid] = s3;
  __syncthreads();
  for (int w = kBoxThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
      red[0][tid] += red[0][tid + w];
      red[1][tid] += red[1][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    sums[0] += red[0][0];
    sums[1] += red[1][0];
    counts[0] += B;
    counts[2] += hist[2 * K];
  }
  for (int k = tid; k < 2 * K; k += kBoxThreads) counts[3 + k] += hist[k];
}

// ---- MeterFrustumKitti.update, metric 'accuracy': counts[0] += B*N, counts[1] += #(argmax(mask_logits, 1) == target) --------------
__global__ __launch_bounds__(kBoxThreads) void frustum_meter_mask_kernel(const float *__restrict__ x, const long long *__restrict__ targets,
                                                                        long long total, int C, int N, long long *counts) {
  __shared__ unsigned hits;
  if (threadIdx.x == 0) hits = 0u;
  __syncthreads();
  unsigned mine = 0u;
  for (long long i = (long long)blockIdx.x * kBoxThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kBoxThreads) {
    const long long b = i / N;
    const int n = (int)(i - b * N);
    const float *row = x + b * C * (long long)N + n;
    float best = row[0];
    int k = 0;
    for (int c = 1; c < C; ++c) {
      const float v = row[(long long)c * N];
      if (v > best || (v != v && best == best)) {
        best = v;
        k = c;
      }
    }
    mine += targets[i] == k ? 1u : 0u;
  }
  if (mine) atomicAdd(&hits, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (hits) atomicAdd(reinterpret_cast<unsigned long long *>(counts + 1), (unsigned long long)hits);
    if (blockIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long *>(counts), (unsigned long long)total);
  }
}

// ---- get_box_iou_3d per pair ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBoxThreads) void box_iou_3d_kernel(const float *__restrict__ c1, const float *__restrict__ ct, int B,
                                                                double *__restrict__ iou_3d, double *__restrict__ iou_2d) {
  const int b = blockIdx.x * kBoxThreads + threadIdx.x;
  if (b >= B) return;
  double i3, i2;
  box_iou_3d(load_corners(c1 + 24ll * b), load_corners(ct + 24ll * b), i3, i2);
  iou_3d[b] = i3;
  iou_2d[b] = i2;
}

// ---- rotate_iou_gpu_eval / d3_box_overlap: an N x K launch of 64 x 64 tiles -----------------------------------------------------------
// rbbox_to_corners: corners (-dx/2, -dy/2), (-dx/2, dy/2), (dx/2, dy/2), (dx/2, -dy/2) turned by the angle,
// x = cos*cx + sin*cy + x0, y = -sin*cx + cos*cy + y0 (fp32).  A tile stages the corners of its 64 boxes and 64 query boxes in LDS
// (plus, for the 3-D overlap, each box's height range and volume in fp64); lane k of a wave takes query box k, so the 64 results a
// wave stores are consecutive in a row of the output.
__device__ __forceinline__ void rbox_corners(const float *__restrict__ r, float (&x)[4], float (&y)[4]) {
  const float a_cos = cosf(r[4]), a_sin = sinf(r[4]);
  const float hx = r[2] / 2.0f, hy = r[3] / 2.0f;
  const float cx[4] = {-hx, -hx, hx, hx}, cy[4] = {-hy, hy, hy, -hy};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[i] = (a_cos * cx[i] + a_sin * cy[i]) + r[0];
    y[i] = (-a_sin * cx[i] + a_cos * cy[i]) + r[1];
  }
}

// criterion of rotate_iou_gpu_eval on one pair: area_q is the query box's (the reference's area1)
__device__ __forceinline__ double bev_value(double inter, double area_q, double area_b, int criterion) {
  return criterion == -1 ? safe_ratio(inter, area_q + area_b - inter)
         : criterion == 0 ? safe_ratio(inter, area_q)
         : criterion == 1 ? safe_ratio(inter, area_b)
                          : inter;
}

// d3_box_overlap_kernel on the fp32 BEV intersection (the reference's rinc), the rest in fp64; (zhi, zlo, vol): a box's height range and
// volume, `b` the box's and `q` the query box's
__device__ __forceinline__ double d3_value(double inter, double zhi_b, double zlo_b, double vol_b, double zhi_q, double zlo_q, double vol_q,
                                           int criterion) {
  const double rinc = (double)(float)inter;
  double v = 0.0;
  if (rinc > 0.0) {
    const double iw = fmin(zhi_b, zhi_q) - fmax(zlo_b, zlo_q);
    if (iw > 0.0) {
      const double area1 = vol_b, area2 = vol_q, inc = iw * rinc;
      v = criterion == -1 ? safe_ratio(inc, area1 + area2 - inc)
          : criterion == 0 ? safe_ratio(inc, area1)
          : criterion == 1 ? safe_ratio(inc, area2)
                           : inc;
    }
  }
  return v;
}

struct TileSide {
  float x[4][kBoxTile], y[4][kBoxTile];
  double zhi[kBoxTile], zlo[kBoxTile], vol[kBoxTile];
};

template <bool kD3>
__device__ __forceinline__ void stage_box(TileSide &side, int lane, long long idx, long long count, const float *__restrict__ bev,
                                          const double *__restrict__ full, int z_axis, double z_center) {
  if (idx >= count) return;
  float x[4], y[4];
  rbox_corners(bev + 5 * idx, x, y);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    side.x[i][lane] = x[i];
    side.y[i][lane] = y[i];
  }
  if (kD3) {
    const double *b = full + 7 * idx;
    side.zhi[lane] = b[z_axis] + b[z_axis + 3] * (1.0 - z_center);
    side.zlo[lane] = b[z_axis] - b[z_axis + 3] * z_center;
    side.vol[lane] = b[3] * b[4] * b[5];
  }
}

template <bool kD3>
__global__ __launch_bounds__(kBoxThreads) void pair_overlap_kernel(const float *__restrict__ bev_b, const double *__restrict__ full_b,
                                                                  long long N, const float *__restrict__ bev_q,
                                                                  const double *__restrict__ full_q, long long K, int criterion,
                                                                  int z_axis, double z_center, float *__restrict__ out) {
  __shared__ TileSide sb, sq;
  const int tid = threadIdx.x, lane = tid & (kBoxTile - 1), row = tid / kBoxTile;
  const long long n0 = (long long)blockIdx.y * kBoxTile, k0 = (long long)blockIdx.x * kBoxTile;
  if (row == 0) stage_box<kD3>(sb, lane, n0 + lane, N, bev_b, full_b, z_axis, z_center);
  if (row == 1) stage_box<kD3>(sq, lane, k0 + lane, K, bev_q, full_q, z_axis, z_center);
  __syncthreads();
  const long long k = k0 + lane;
  if (k >= K) return;
  float qx[4], qy[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    qx[i] = sq.x[i][lane];
    qy[i] = sq.y[i][lane];
  }
  for (int r = row; r < kBoxTile; r += kBoxThreads / kBoxTile) {
    const long long n = n0 + r;
    if (n >= N) break;
    float bx[4], by[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bx[i] = sb.x[i][r];
      by[i] = sb.y[i][r];
    }
    // the reference evaluates dev_rotate_iou_eval(query_boxes[k], boxes[n]): area1 is the query box's
    double area_q, area_b;
    const double inter = quad_overlap(qx, qy, bx, by, area_q, area_b);
    const double v = !kD3 ? bev_value(inter, area_q, area_b, criterion)
                          : d3_value(inter, sb.zhi[r], sb.zlo[r], sb.vol[r], sq.zhi[lane], sq.zlo[lane], sq.vol[lane], criterion);
    out[n * K + k] = (float)v;
  }
}

// ---- the same overlaps over ragged per-image blocks (the KITTI AP evaluation reads only the diagonal blocks of the reference's
// 50-image N x K parts): image i holds boxes b_off[i] .. b_off[i+1] and query boxes q_off[i] .. q_off[i+1]; its (boxes_i, queries_i)
// row-major block starts at out[pair_off[i]].  One lane per pair; the image of a pair is found by bisection of pair_off.
template <bool kD3>
__global__ __launch_bounds__(kBoxThreads) void segmented_overlap_kernel(const float *__restrict__ bev_b, const double *__restrict__ full_b,
                                                                       const float *__restrict__ bev_q, const double *__restrict__ full_q,
                                                                       const long long *__restrict__ b_off, const long long *__restrict__ q_off,
                                                                       const long long *__restrict__ pair_off, long long images,
                                                                       long long total, int criterion, int z_axis, double z_center,
                                                                       float *__restrict__ out) {
  const long long p = (long long)blockIdx.x * kBoxThreads + threadIdx.x;
  if (p >= total) return;
  long long lo = 0, hi = images;                       // the last image with pair_off[i] <= p
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (pair_off[mid] <= p) lo = mid; else hi = mid;
  }
  const long long nb = b_off[lo + 1] - b_off[lo], nq = q_off[lo + 1] - q_off[lo], r = p - pair_off[lo];
  if (nq <= 0 || r >= nb * nq) return;
  const long long n = b_off[lo] + r / nq, k = q_off[lo] + r % nq;
  float bx[4], by[4], qx[4], qy[4];
  rbox_corners(bev_b + 5 * n, bx, by);
  rbox_corners(bev_q + 5 * k, qx, qy);
  double area_q, area_b;
  const double inter = quad_overlap(qx, qy, bx, by, area_q, area_b);
  double v;
  if (!kD3) {
    v = bev_value(inter, area_q, area_b, criterion);
  } else {
    const double *b = full_b + 7 * n, *q = full_q + 7 * k;
    v = d3_value(inter, b[z_axis] + b[z_axis + 3] * (1.0 - z_center), b[z_axis] - b[z_axis + 3] * z_center, b[3] * b[4] * b[5],
                 q[z_axis] + q[z_axis + 3] * (1.0 - z_center), q[z_axis] - q[z_axis + 3] * z_center, q[3] * q[4] * q[5], criterion);
  }
  out[p] = (float)v;
}

// ---- update_predictions (evaluate/kitti/frustum/eval.py:227-244) on the decoded boxes, fp64 ------------------------------------------
__global__ __launch_bounds__(kBoxThreads) void frustum_predictions_kernel(BoxHeads o, int B, int NH, int NS,
                                                                         const float *__restrict__ bin_centers,
                                                                         const float *__restrict__ templates,
                                                                         const double *__restrict__ rotation_angle,
                                                                         const double *__restrict__ rgb_score, double *__restrict__ table,
                                                                         long long rows, long long step) {
  const int b = blockIdx.x * kBoxThreads + threadIdx.x;
  if (b >= B || step + b < 0 || step + b >= rows) return;
  float heading, size[3];
  decode_prediction(o, b, NH, NS, bin_centers, templates, heading, size);
  const double l = size[0], w = size[1], h = size[2];
  const double x = o.center[3 * b], y = o.center[3 * b + 1], z = o.center[3 * b + 2];
  double r = rotation_angle[b];
  const double v_cos = cos(r), v_sin = sin(r);
  const double cx = v_cos * x + v_sin * z;
  const double cy = y + h / 2.0;
  const double cz = v_cos * z - v_sin * x;
  r = r + (double)heading;
  for (int i = 0; i < kWrapCap && r > M_PI; ++i) r = r - 2 * M_PI;
  for (int i = 0; i < kWrapCap && r < -M_PI; ++i) r = r + 2 * M_PI;
  double *p = table + (step + b) * 8;
  p[0] = h;
  p[1] = w;
  p[2] = l;
  p[3] = cx;
  p[4] = cy;
  p[5] = cz;
  p[6] = r;
  p[7] = rgb_score[b];
}

}  // namespace pvcnn

using namespace pvcnn;

extern "C" int pvcnn_frustum_meter_update(const float *center, const float *heading_scores, const float *heading_residuals,
                                          const float *size_scores, const float *size_residuals, const float *center_t,
                                          const long long *heading_bin_id_t, const float *heading_residual_t,
                                          const long long *size_template_id_t, const float *size_residual_t, const long long *class_id_t,
                                          int B, int NH, int NS, const float *bin_centers, const float *size_templates,
                                          const long long *class_ids, const double *thresholds, int num_classes, const float *mask_logits,
                                          const long long *mask_targets, int C, int N, double *sums, long long *counts, void *stream) {
  PVCNN_REQUIRE(B >= 0, "bad batch size");
  PVCNN_REQUIRE(counts != nullptr, "null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mask_logits != nullptr) {
    PVCNN_REQUIRE(C > 0 && N >= 0, "bad mask sizes");
    const long long total = (long long)B * N;
    if (total == 0) return 0;
    PVCNN_REQUIRE(mask_targets != nullptr, "null pointer");
    const unsigned grid = (unsigned)std::min<long long>((total + kBoxThreads - 1) / kBoxThreads, 1024);
    hipLaunchKernelGGL(frustum_meter_mask_kernel, dim3(grid), dim3(kBoxThreads), 0, s, mask_logits, mask_targets, total, C, N, counts);
    return check_launch("frustum_meter_mask");
  }
  PVCNN_REQUIRE(NH > 0 && NS > 0, "NH and NS must be > 0");
  PVCNN_REQUIRE(num_classes >= 0 && num_classes <= kBoxMaxClasses, "num_classes must be in [0, 64]");
  if (B == 0) return 0;
  PVCNN_REQUIRE(center && heading_scores && heading_residuals && size_scores && size_residuals && center_t && heading_bin_id_t &&
                    heading_residual_t && size_template_id_t && size_residual_t && class_id_t && bin_centers && size_templates && sums,
                "null pointer");
  PVCNN_REQUIRE(num_classes == 0 || (class_ids && thresholds), "null class table");
  const BoxHeads o{center, heading_scores, heading_residuals, size_scores, size_residuals};
  const MeterTargets t{center_t, heading_residual_t, size_residual_t, heading_bin_id_t, size_template_id_t, class_id_t};
  hipLaunchKernelGGL(frustum_meter_box_kernel, dim3(1), dim3(kBoxThreads), 0, s, o, t, B, NH, NS, bin_centers, size_templates, class_ids,
                     thresholds, num_classes, sums, counts);
  return check_launch("frustum_meter_box");
}

extern "C" int pvcnn_box_iou_3d(const float *corners_1, const float *corners_t, int B, double *iou_3d, double *iou_2d, void *stream) {
  PVCNN_REQUIRE(B >= 0, "bad batch size");
  if (B == 0) return 0;
  PVCNN_REQUIRE(corners_1 && corners_t && iou_3d && iou_2d, "null pointer");
  hipLaunchKernelGGL(box_iou_3d_kernel, dim3((unsigned)ceil_div(B, kBoxThreads)), dim3(kBoxThreads), 0, static_cast<hipStream_t>(stream),
                     corners_1, corners_t, B, iou_3d, iou_2d);
  return check_launch("box_iou_3d");
}

static int launch_pair_overlap(const float *bev_b, const double *full_b, long long N, const float *bev_q, const double *full_q,
                               long long K, int criterion, int z_axis, double z_center, float *out, void *stream) {
  PVCNN_REQUIRE(N >= 0 && K >= 0, "bad sizes");
  if (N == 0 || K == 0) return 0;
  const long long tiles_n = (N + kBoxTile - 1) / kBoxTile, tiles_k = (K + kBoxTile - 1) / kBoxTile;
  PVCNN_REQUIRE(tiles_n <= 65535 && tiles_k < (1ll << 31), "N must be <= 65535 * 64");
  PVCNN_REQUIRE(bev_b && bev_q && out, "null pointer");
  const dim3 grid((unsigned)tiles_k, (unsigned)tiles_n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (full_b == nullptr) {
    hipLaunchKernelGGL(pair_overlap_kernel<false>, grid, dim3(kBoxThreads), 0, s, bev_b, nullptr, N, bev_q, nullptr, K, criterion, 0, 0.0,
                       out);
    return check_launch("rotate_iou");
  }
  hipLaunchKernelGGL(pair_overlap_kernel<true>, grid, dim3(kBoxThreads), 0, s, bev_b, full_b, N, bev_q, full_q, K, criterion, z_axis,
                     z_center, out);
  return check_launch("box3d_overlap");
}

extern "C" int pvcnn_rotate_iou(const float *boxes, long long N, const float *query_boxes, long long K, int criterion, float *out,
                                void *stream) {
  return launch_pair_overlap(boxes, nullptr, N, query_boxes, nullptr, K, criterion, 0, 0.0, out, stream);
}

extern "C" int pvcnn_box3d_overlap(const float *bev_boxes, const double *boxes, long long N, const float *bev_query_boxes,
                                   const double *query_boxes, long long K, int criterion, int z_axis, double z_center, float *out,
                                   void *stream) {
  PVCNN_REQUIRE(z_axis >= 0 && z_axis <= 2, "z_axis must be 0, 1 or 2");
  PVCNN_REQUIRE(N == 0 || K == 0 || (boxes && query_boxes), "null pointer");
  return launch_pair_overlap(bev_boxes, boxes, N, bev_query_boxes, query_boxes, K, criterion, z_axis, z_center, out, stream);
}

extern "C" int pvcnn_kitti_ap_box_overlaps(const float *bev_boxes, const double *boxes, const float *bev_query_boxes,
                                           const double *query_boxes, const long long *box_off, const long long *query_off,
                                           const long long *pair_off, long long images, long long total_pairs, int criterion, int z_axis,
                                           double z_center, float *out, void *stream) {
  PVCNN_REQUIRE(images >= 0 && total_pairs >= 0, "bad sizes");
  PVCNN_REQUIRE(z_axis >= 0 && z_axis <= 2, "z_axis must be 0, 1 or 2");
  PVCNN_REQUIRE((boxes == nullptr) == (query_boxes == nullptr), "boxes and query_boxes go together");
  if (images == 0 || total_pairs == 0) return 0;
  PVCNN_REQUIRE(bev_boxes && bev_query_boxes && box_off && query_off && pair_off && out, "null pointer");
  const long long blocks = (total_pairs + kBoxThreads - 1) / kBoxThreads;
  PVCNN_REQUIRE(blocks < (1ll << 31), "too many pairs");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (boxes == nullptr) {
    hipLaunchKernelGGL(segmented_overlap_kernel<false>, dim3((unsigned)blocks), dim3(kBoxThreads), 0, s, bev_boxes, nullptr,
                       bev_query_boxes, nullptr, box_off, query_off, pair_off, images, total_pairs, criterion, 0, 0.0, out);
  } else {
    hipLaunchKernelGGL(segmented_overlap_kernel<true>, dim3((unsigned)blocks), dim3(kBoxThreads), 0, s, bev_boxes, boxes, bev_query_boxes,
                       query_boxes, box_off, query_off, pair_off, images, total_pairs, criterion, z_axis, z_center, out);
  }
  return check_launch("kitti_ap_box_overlaps");
}

extern "C" int pvcnn_frustum_predictions(const float *center, const float *heading_scores, const float *heading_residuals,
                                         const float *size_scores, const float *size_residuals, int B, int NH, int NS,
                                         const float *bin_centers, const float *size_templates, const double *rotation_angle,
                                         const double *rgb_score, double *table, long long rows, long long step, void *stream) {
  PVCNN_REQUIRE(B >= 0 && NH > 0 && NS > 0 && rows >= 0 && step >= 0, "bad sizes");
  PVCNN_REQUIRE(step + B <= rows, "the batch does not fit in the table at current_step");
  if (B == 0) return 0;
  PVCNN_REQUIRE(center && heading_scores && heading_residuals && size_scores && size_residuals && bin_centers && size_templates &&
                    rotation_angle && rgb_score && table,
                "null pointer");
  const BoxHeads o{center, heading_scores, heading_residuals, size_scores, size_residuals};
  hipLaunchKernelGGL(frustum_predictions_kernel, dim3((unsigned)ceil_div(B, kBoxThreads)), dim3(kBoxThreads), 0,
                     static_cast<hipStream_t>(stream), o, B, NH, NS, bin_centers, size_templates, rotation_angle, rgb_score, table, rows,
                     step);
  return check_launch("frustum_predictions");
}
