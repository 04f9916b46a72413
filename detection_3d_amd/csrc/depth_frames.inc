// A batch of posed depth frames as the kernels of unproject.hip and tsdf.hip read it: the depth of a pixel, which
// depths count as a measurement, which pixels a call keeps, and the camera of a frame.  The arithmetic is the contract
// of include/d3d_hip.h (d3d_unproject_*); both files, and render.hip for the camera and the frames it fills, include this
// one so that there is one definition of it, and one host-side check of a d3d_depth_frames.
// Included inside namespace d3d's anonymous namespace.

struct DepthView {
  const void *depth;
  int is_u16, H, W, step;
  long P;                                    // frames * H * W < 2^31
  double scale, zmin, zmax;
};

__device__ __forceinline__ double depth_at(const DepthView &V, long p) {
  return V.is_u16 ? (double)((const uint16_t *)V.depth)[p] * V.scale : (double)((const float *)V.depth)[p];
}
__device__ __forceinline__ bool valid_z(const DepthView &V, double z) {
  return z > 0.0 && z < (double)INFINITY && z >= V.zmin && z <= V.zmax;     // false for NaN
}

// pixel p of the batch: (f, v, u), and whether it is kept (z: its depth when it is)
__device__ __forceinline__ bool kept_at(const DepthView &V, long p, int &f, int &v, int &u, double &z) {
  if (p >= V.P) return false;
  const int row = (int)(p / V.W);
  u = (int)(p - (long)row * V.W);
  f = row / V.H;
  v = row - f * V.H;
  if (V.step > 1 && (u % V.step != 0 || v % V.step != 0)) return false;
  z = depth_at(V, p);
  return valid_z(V, z);
}

struct Camera {
  double fx, fy, cx, cy, R[3][3], t[3];
};

// frame f of intrinsics fp64 [F, 4] (fx, fy, cx, cy) and extrinsics fp64 [F, 3, 4] (R | t)
__device__ __forceinline__ void load_camera(const double *__restrict__ intr, const double *__restrict__ extr, int f,
                                            Camera &K) {
  K.fx = intr[4 * f + 0];
  K.fy = intr[4 * f + 1];
  K.cx = intr[4 * f + 2];
  K.cy = intr[4 * f + 3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
#pragma unroll
    for (int j = 0; j < 3; j++) K.R[k][j] = extr[12 * f + 4 * k + j];
    K.t[k] = extr[12 * f + 4 * k + 3];
  }
}

__device__ __forceinline__ void cam_point(const Camera &K, int u, int v, double z, double (&C)[3]) {
  const double zx = z / K.fx, zy = z / K.fy;
  C[0] = ((double)u - K.cx) * zx;
  C[1] = ((double)v - K.cy) * zy;
  C[2] = z;
}

// ---- the host's check of a d3d_depth_frames ----

enum { kFramesDepth = 1, kFramesCameras = 2 };   // what a call reads of a batch that has pixels

// the descriptor's shape -> its pixels; D3D_OK with P == 0 for an empty batch
inline int frames_shape(const char *who, const d3d_depth_frames *F, long &P) {
  D3D_REQUIRE(F, "%s: null pointer", who);
  D3D_REQUIRE(F->frames >= 0 && F->height >= 1 && F->width >= 1, "%s: %d frames of %d x %d pixels", who, F->frames,
              F->height, F->width);
  const double pixels = (double)F->frames * (double)F->height * (double)F->width;
  D3D_REQUIRE(pixels < 2147483648.0, "%s: %d x %d x %d = %.0f pixels do not fit 31 bits (use fewer frames per call)", who,
              F->frames, F->height, F->width, pixels);
  P = (long)pixels;
  return D3D_OK;
}

// the checked descriptor and the call's own choices -> the view; `needs`: the pointers that must not be null when P > 0
inline int frames_view(const char *who, const d3d_depth_frames *F, int step, double min_depth, double max_depth, int needs,
                       DepthView &V) {
  long P = 0;
  const int rc = frames_shape(who, F, P);
  if (rc) return rc;
  D3D_REQUIRE(step >= 1, "%s: step %d < 1", who, step);
  D3D_REQUIRE(!F->depth_is_u16 || (F->depth_scale > 0.0 && F->depth_scale < (double)INFINITY),
              "%s: depth_scale %g must be positive and finite", who, F->depth_scale);
  D3D_REQUIRE(min_depth == min_depth && max_depth == max_depth, "%s: min_depth / max_depth is NaN", who);
  D3D_REQUIRE(P == 0 || ((!(needs & kFramesDepth) || F->depth) && (!(needs & kFramesCameras) || (F->intrinsics && F->extrinsics))),
              "%s: null pointer", who);
  V = DepthView{F->depth, F->depth_is_u16 ? 1 : 0, F->height, F->width, step, P, F->depth_scale, min_depth, max_depth};
  return D3D_OK;
}
