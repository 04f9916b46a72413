// Rotated BEV IoU x z-interval IoU of two boxes (consumers: box_match.hip, nms.hip).  Included inside namespace d3d.
//
// Arithmetic contract (shared with the oracle, compiled with -ffp-contract=off): fp32 for the
// geometry of second/core/non_max_suppression/nms_gpu.py, fp64 for the triangle-fan sum and the
// final ratio (numba promotes `x / 2.0`), cos/sin evaluated in fp64 and rounded to fp32.

struct Quad {
  float p[8];  // 4 corners (x,y), order of rbbox_to_corners (nms_gpu.py:355-378)
};

__device__ __forceinline__ Quad make_quad(float xc, float yc, float xd, float yd, float angle) {
  const float a_cos = (float)cos((double)angle);
  const float a_sin = (float)sin((double)angle);
  const float cx[4] = {-xd / 2, -xd / 2, xd / 2, xd / 2};
  const float cy[4] = {-yd / 2, yd / 2, yd / 2, -yd / 2};
  Quad q;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    q.p[2 * i] = a_cos * cx[i] + a_sin * cy[i] + xc;
    q.p[2 * i + 1] = -a_sin * cx[i] + a_cos * cy[i] + yc;
  }
  return q;
}

// nms_gpu.py:310-328
__device__ __forceinline__ bool point_in_quad(float px, float py, const float *c) {
  const float ab0 = c[2] - c[0], ab1 = c[3] - c[1];
  const float ad0 = c[6] - c[0], ad1 = c[7] - c[1];
  const float ap0 = px - c[0], ap1 = py - c[1];
  const float abab = ab0 * ab0 + ab1 * ab1;
  const float abap = ab0 * ap0 + ab1 * ap1;
  const float adad = ad0 * ad0 + ad1 * ad1;
  const float adap = ad0 * ap0 + ad1 * ap1;
  return abab >= abap && abap >= 0 && adad >= adap && adap >= 0;
}

// nms_gpu.py:222-265
__device__ __forceinline__ bool seg_intersect(const float *p1, const float *p2, int i, int j,
                                              float *out) {
  const float A0 = p1[2 * i], A1 = p1[2 * i + 1];
  const float B0 = p1[2 * ((i + 1) & 3)], B1 = p1[2 * ((i + 1) & 3) + 1];
  const float C0 = p2[2 * j], C1 = p2[2 * j + 1];
  const float D0 = p2[2 * ((j + 1) & 3)], D1 = p2[2 * ((j + 1) & 3) + 1];
  const float BA0 = B0 - A0, BA1 = B1 - A1;
  const float DA0 = D0 - A0, CA0 = C0 - A0;
  const float DA1 = D1 - A1, CA1 = C1 - A1;
  const bool acd = DA1 * CA0 > CA1 * DA0;
  const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
  if (acd == bcd) return false;
  const bool abc = CA1 * BA0 > BA1 * CA0;
  const bool abd = DA1 * BA0 > BA1 * DA0;
  if (abc == abd) return false;
  const float DC0 = D0 - C0, DC1 = D1 - C1;
  const float ABBA = A0 * B1 - B0 * A1;
  const float CDDC = C0 * D1 - D0 * C1;
  const float DH = BA1 * DC0 - BA0 * DC1;
  const float Dx = ABBA * DC0 - BA0 * CDDC;
  const float Dy = ABBA * DC1 - BA1 * CDDC;
  out[0] = Dx / DH;
  out[1] = Dy / DH;
  return true;
}

// The point list (up to 24 points) and the sort keys of inter() are indexed at run time: as private arrays they live in
// scratch memory.  PrivatePts is that form; LdsPts keeps them in a column of LDS the caller provides (element i of
// thread t at base[i * stride + t]) -- same operations in the same order.
struct PrivatePts {
  float p[48], v[24];
  __device__ __forceinline__ float &pt(int i) { return p[i]; }
  __device__ __forceinline__ float &key(int i) { return v[i]; }
};
struct LdsPts {
  float *base;
  int stride;
  __device__ __forceinline__ float &pt(int i) { return base[i * stride]; }
  __device__ __forceinline__ float &key(int i) { return base[(48 + i) * stride]; }
};
static constexpr int kLdsPtsFloats = 72;

// inter() of nms_gpu.py:381-395 on precomputed corners: q1 = rbbox1, q2 = rbbox2.
template <class Pts>
__device__ double quad_inter_f32(const Quad &q1, const Quad &q2, Pts B) {
  int num = 0;
  // nms_gpu.py:331-352
  for (int i = 0; i < 4; i++) {
    if (point_in_quad(q1.p[2 * i], q1.p[2 * i + 1], q2.p)) {
      B.pt(num * 2) = q1.p[2 * i];
      B.pt(num * 2 + 1) = q1.p[2 * i + 1];
      num++;
    }
    if (point_in_quad(q2.p[2 * i], q2.p[2 * i + 1], q1.p)) {
      B.pt(num * 2) = q2.p[2 * i];
      B.pt(num * 2 + 1) = q2.p[2 * i + 1];
      num++;
    }
  }
  float tmp[2];
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      if (seg_intersect(q1.p, q2.p, i, j, tmp)) {
        B.pt(num * 2) = tmp[0];
        B.pt(num * 2 + 1) = tmp[1];
        num++;
      }
  if (num < 3) return 0.0;
  // nms_gpu.py:182-219
  float cx = 0.f, cy = 0.f;
  for (int i = 0; i < num; i++) {
    cx += B.pt(2 * i);
    cy += B.pt(2 * i + 1);
  }
  cx = (float)((double)cx / num);
  cy = (float)((double)cy / num);
  for (int i = 0; i < num; i++) {
    float v0 = B.pt(2 * i) - cx, v1 = B.pt(2 * i + 1) - cy;
    const float d = sqrtf(v0 * v0 + v1 * v1);
    v0 = v0 / d;
    v1 = v1 / d;
    if (v1 < 0) v0 = -2 - v0;
    B.key(i) = v0;
  }
  for (int i = 1; i < num; i++) {
    if (B.key(i - 1) > B.key(i)) {
      const float temp = B.key(i), tx = B.pt(2 * i), ty = B.pt(2 * i + 1);
      int j = i;
      while (j > 0 && B.key(j - 1) > temp) {
        B.key(j) = B.key(j - 1);
        B.pt(j * 2) = B.pt(j * 2 - 2);
        B.pt(j * 2 + 1) = B.pt(j * 2 - 1);
        j--;
      }
      B.key(j) = temp;
      B.pt(j * 2) = tx;
      B.pt(j * 2 + 1) = ty;
    }
  }
  // nms_gpu.py:166-179
  double area = 0.0;
  for (int i = 0; i < num - 2; i++) {
    const float a0 = B.pt(0), a1 = B.pt(1), b0 = B.pt(2 * i + 2), b1 = B.pt(2 * i + 3), c0 = B.pt(2 * i + 4),
                c1 = B.pt(2 * i + 5);
    const float v = (a0 - c0) * (b1 - c1) - (a1 - c1) * (b0 - c0);
    area += fabs((double)v / 2.0);
  }
  return area;
}

// devRotateIoUEval (nms_gpu.py:552-570): rbox1 = (q1, dims d1a x d1b), rbox2 likewise.
// `disjoint`: the caller knows that the quads' bounding boxes are strictly apart -- then inter() finds no corner inside
// the other quad and no edge crossing, i.e. returns exactly 0.0, and only the criterion's formula is left to evaluate
template <class Pts = PrivatePts>
__device__ __forceinline__ float iou_eval(const Quad &q1, float d1a, float d1b, const Quad &q2,
                                          float d2a, float d2b, int criterion, Pts B = Pts(), bool disjoint = false) {
  const float area1 = d1a * d1b, area2 = d2a * d2b;
  const double ai = disjoint ? 0.0 : quad_inter_f32(q1, q2, B);
  if (criterion == -1) return (float)(ai / ((double)(area1 + area2) - ai));
  if (criterion == 0) return (float)(ai / area1);
  if (criterion == 1) return (float)(ai / area2);
  if (criterion == 2) {
    const bool small = fminf(d2a, d2b) / fmaxf(d2a, d2b) < 0.25;
    if (small) return (float)(ai / ((double)area2 + fmax(0.0, (double)area1 * 0.5 - ai)));
    return (float)(ai / ((double)(area1 + area2) - ai));
  }
  return (float)ai;
}

// fp64 Sutherland-Hodgman clip of quad P by quad Q (both fp32 corners); returns the area.
// The two vertex lists (a quad clipped by four half-planes has at most 8 vertices) are indexed at run time; as private
// arrays they end up in scratch memory (528 B per lane, every access a round trip), so the caller hands in a column of
// LDS instead: element i of list l of thread t is buf[(l * 16 + i) * stride + t].  Same operations in the same order.
__device__ __forceinline__ double quad_inter_f64(const float *P, const float *Q, double *buf, int stride) {
  double *a = buf, *b = buf + 16 * stride;
  int na = 4;
#pragma unroll
  for (int i = 0; i < 8; i++) a[i * stride] = P[i];
  double sq = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int j = (i + 1) & 3;
    sq += (double)Q[2 * i] * Q[2 * j + 1] - (double)Q[2 * j] * Q[2 * i + 1];
  }
  const double sgn = sq >= 0 ? 1.0 : -1.0;
#pragma unroll
  for (int e = 0; e < 4; e++) {      // (unrolled: Q is then indexed statically and stays in registers)
    if (na <= 0) break;
    const double x1 = Q[2 * e], y1 = Q[2 * e + 1];
    const double x2 = Q[2 * ((e + 1) & 3)], y2 = Q[2 * ((e + 1) & 3) + 1];
    int nb = 0;
    for (int i = 0; i < na; i++) {
      const int j = (i + 1) % na;
      const double cx = a[(2 * i) * stride], cy = a[(2 * i + 1) * stride], nx = a[(2 * j) * stride],
                   ny = a[(2 * j + 1) * stride];
      const double dc = sgn * ((x2 - x1) * (cy - y1) - (y2 - y1) * (cx - x1));
      const double dn = sgn * ((x2 - x1) * (ny - y1) - (y2 - y1) * (nx - x1));
      if (dc >= 0) {
        b[(2 * nb) * stride] = cx;
        b[(2 * nb + 1) * stride] = cy;
        nb++;
      }
      if ((dc >= 0) != (dn >= 0)) {
        const double t = dc / (dc - dn);
        b[(2 * nb) * stride] = cx + t * (nx - cx);
        b[(2 * nb + 1) * stride] = cy + t * (ny - cy);
        nb++;
      }
    }
    na = nb;
    double *tmp = a;   // the clipped list is the next edge's input
    a = b;
    b = tmp;
  }
  if (na < 3) return 0.0;
  double s = 0;
  for (int i = 0; i < na; i++) {
    const int j = (i + 1) % na;
    s += a[(2 * i) * stride] * a[(2 * j + 1) * stride] - a[(2 * j) * stride] * a[(2 * i + 1) * stride];
  }
  return fabs(s) * 0.5;
}
__device__ __forceinline__ double quad_area_f64(const float *P) {
  double s = 0;
  for (int i = 0; i < 4; i++) {
    const int j = (i + 1) & 3;
    s += (double)P[2 * i] * P[2 * j + 1] - (double)P[2 * j] * P[2 * i + 1];
  }
  return fabs(s) * 0.5;
}

// ------------------------------------------------------------------------------------------
// One entry of an IoU matrix (k_iou_matrix, label assignment).
// mode 0: rotate_iou_gpu_eval on [*,5] boxes.  mode 1: boxes_iou_3d on [*,7] yx_zb boxes.
struct IouArgs {
  const float *rows;  // "boxes"/"targets"  [N, stride]
  const float *cols;  // "query"/"anchors"  [K, stride]
  int N, K, mode, criterion, only_xy;
  float aug[4];
  float *out;
};
struct BoxRec {
  Quad q;
  float d0, d1, z0, z1;
  float raw[5];
  float lo[2], hi[2];   // bounding box of the corners
};
__device__ __forceinline__ void load_box(const IouArgs &a, const float *base, int idx, bool is_row,
                                         BoxRec &r) {
  float xc, yc, d0, d1, ang;
  if (a.mode == 0) {
    const float *b = base + (size_t)idx * 5;
    xc = b[0]; yc = b[1]; d0 = b[2]; d1 = b[3]; ang = b[4];
    r.z0 = 0.f; r.z1 = 1.f;
  } else {
    const float *b = base + (size_t)idx * 7;
    const float cy = is_row ? a.aug[0] : a.aug[2], cz = is_row ? a.aug[1] : a.aug[3];
    // torch.clamp(min=) of boxes_iou_3d: a NaN size stays NaN (fmaxf would replace it by the bound)
    xc = b[0]; yc = b[1]; d0 = b[3] < cy ? cy : b[3]; d1 = b[4]; ang = b[6];
    const float dz = b[5] < cz ? cz : b[5];
    r.z0 = b[2];
    r.z1 = b[2] + dz;  // rotate_nms_3d_torch.py:15-16
  }
  r.d0 = d0; r.d1 = d1;
  r.raw[0] = xc; r.raw[1] = yc; r.raw[2] = d0; r.raw[3] = d1; r.raw[4] = ang;
  r.q = make_quad(xc, yc, d0, d1, ang);
#pragma unroll
  for (int d = 0; d < 2; d++) {
    r.lo[d] = fminf(fminf(r.q.p[d], r.q.p[2 + d]), fminf(r.q.p[4 + d], r.q.p[6 + d]));
    r.hi[d] = fmaxf(fmaxf(r.q.p[d], r.q.p[2 + d]), fmaxf(r.q.p[4 + d], r.q.p[6 + d]));
  }
  // point_in_quad takes a point as inside when its projections on the edges AB and AD fall within them.  An edge without
  // length (a size of 0) bounds nothing: corners of a box far away count as inside, and inter() of such a pair is not 0.
  // A box with such an edge gets a NaN bounding box, so that iou_pair's early-out never applies to it.
  const float ab0 = r.q.p[2] - r.q.p[0], ab1 = r.q.p[3] - r.q.p[1], ad0 = r.q.p[6] - r.q.p[0], ad1 = r.q.p[7] - r.q.p[1];
  if (!(ab0 * ab0 + ab1 * ab1 > 0.f && ad0 * ad0 + ad1 * ad1 > 0.f))
    r.lo[0] = r.lo[1] = r.hi[0] = r.hi[1] = __builtin_nanf("");
}

// one entry of the matrix: row box rb (target / "boxes"), column box cb (anchor / "query")
__device__ __forceinline__ float iou_pair(const IouArgs &a, const BoxRec &rb, const BoxRec &cb) {
  // kernel order (nms_gpu.py:605-611): rbox1 = query (col), rbox2 = box (row).  Most pairs of an anchors x targets
  // matrix are far apart: their bounding boxes do not touch and the intersection is exactly 0 (NaN corners and the NaN
  // bounds of a box with a zero size compare false and take the full path)
  const bool apart = cb.hi[0] < rb.lo[0] || rb.hi[0] < cb.lo[0] || cb.hi[1] < rb.lo[1] || rb.hi[1] < cb.lo[1];
  float v = iou_eval(cb.q, cb.d0, cb.d1, rb.q, rb.d0, rb.d1, a.criterion, PrivatePts(), apart);
  bool same = true;  // check_same_boxes, nms_gpu.py:653-664
#pragma unroll
  for (int d = 0; d < 5; d++) same = same && (fabsf(rb.raw[d] - cb.raw[d]) < (float)1e-6);
  if (same) v = 1.f;
  if (a.mode == 1 && !a.only_xy) {
    // iou_one_dim's torch.min / torch.max (rotate_nms_3d_torch.py:18-19): a NaN bound makes overlap and common NaN (fminf /
    // fmaxf would drop it).  z0 = NaN or dz = NaN both leave z1 = NaN, so testing z1 covers the box.
    const bool znan = cb.z1 != cb.z1 || rb.z1 != rb.z1;
    const float overlap = fminf(cb.z1, rb.z1) - fmaxf(cb.z0, rb.z0);
    const float common = fmaxf(cb.z1, rb.z1) - fminf(cb.z0, rb.z0);
    v = v * (znan ? __builtin_nanf("") : overlap / common);
  }
  return v;
}
