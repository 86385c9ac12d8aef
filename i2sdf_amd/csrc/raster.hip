// Mesh depth on the device: the camera-space z of the nearest triangle along every pixel's ray, for a list of pinhole cameras --
// what utils/mesh_util.py:refuse gets from pyrender (an OpenGL depth render read back on the host) before it fuses the depth maps.
//
// Camera convention (rend_util.load_K_Rt_from_P): x right, y down, z forward; pixel (u, v) = column, row; the sample of a pixel
// is the ray through d = ((u - cx) / fx, (v - cy) / fy, 1).  depth[c, v, u] = z of the nearest hit with znear <= z <= zfar, 0 for none.
//
// Arithmetic (every product and sum rounded on its own, in the order written; tests/refuse_ref.py follows it):
//   project   fp32, once per (camera, vertex): q_k = ((w[4k] x + w[4k+1] y) + w[4k+2] z) + w[4k+3], w = the camera's world-to-camera
//             rows (3 x 4, row major).
//   setup     fp64 from the fp32 camera-space vertices a, b, c (the products of two fp32 numbers are exact in fp64):
//               n0 = b x c, n1 = c x a, n2 = a x b   (cross(p, q).x = p.y q.z - p.z q.y, cyclic)
//               det = (a.x n0.x + a.y n0.y) + a.z n0.z          = a . (b - a) x (c - a): negative when the triangle's right-hand
//                                                                 normal points at the camera (counter-clockwise as the camera sees it)
//             det == 0 (or NaN): nothing.  det > 0 is a back face: dropped with cull, kept as it is without.  det < 0: n_i and det
//             are negated.  From here det > 0 and the inside of the triangle is where every edge function is positive.
//   sample    fp64: dx = ((double)u - cx) / fx, dy = ((double)v - cy) / fy, e_i = (n_i.x dx + n_i.y dy) + n_i.z.
//             Covered iff every e_i > 0, or e_i == 0 on an edge with n_i.x > 0 (a left edge), or n_i.x == 0 and n_i.y > 0 (a top
//             edge).  Two triangles that share an edge compute exactly negated n_i and e_i there, so each sample goes to one of them.
//             s = (e0 + e1) + e2 (> 0), z = (float)(det / s): the ray-plane intersection, which is what perspective-correct
//             interpolation of z gives.  A sample with z outside [znear, zfar] is discarded -- samples, not triangles, so a triangle
//             that crosses the camera plane still covers the pixels of its part in front (nothing is divided by a vertex's z).
//   visibility  positive floats order like their bit patterns: a 32-bit unsigned atomicMin per covered sample.  The image does not
//             depend on the order in which triangles arrive.
//   box       only has to be conservative: the fp32 pixel box ((x fx) / z + cx, (y fy) / z + cy) of the triangle clipped against
//             z = znear (vertices behind it are replaced by the crossings of their edges), widened by one pixel, cut to the image.
// Two populations, split by box area (I2SDF_RASTER_SMALL_MAX pixels):
//   rs_small  one lane per (camera, triangle): walks a small box itself (marching-cubes triangles are below a pixel); a larger one is
//             appended to the camera's list (an integer atomic; the list's order varies from run to run, the image does not);
//   rs_large  one 256-thread workgroup per listed triangle strides over its box (a wall of a ground-truth mesh covers the image).
// Cameras are processed in chunks that fit the workspace (projected vertices + list); the depth maps of all cameras stay resident.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/i2sdf.h"

#pragma clang fp contract(off)

int i2sdf_hip_check(hipError_t e, const char* what);

namespace {

constexpr int RS_THREADS = 256;
constexpr int64_t RS_BUDGET = (int64_t)256 << 20;    // bytes of workspace a chunk of cameras may take (one camera always fits)
constexpr int RS_LARGE_BLOCKS = 2048;                // workgroups per camera that stride over its list
constexpr uint32_t RS_EMPTY = 0xFFFFFFFFu;

struct Cam {
  float fx, fy, cx, cy, znear, zfar;
  int H, W, cull;
};

struct Tri {
  double n[3][3];
  double det;
  int x0, x1, y0, y1;
};

__device__ __forceinline__ void cross64(const double p[3], const double q[3], double o[3]) {
  o[0] = p[1] * q[2] - p[2] * q[1];
  o[1] = p[2] * q[0] - p[0] * q[2];
  o[2] = p[0] * q[1] - p[1] * q[0];
}

__device__ __forceinline__ void box_add(const Cam& C, float x, float y, float z, float lo[2], float hi[2]) {
  const float px = (x * C.fx) / z + C.cx, py = (y * C.fy) / z + C.cy;
  lo[0] = fminf(lo[0], px); hi[0] = fmaxf(hi[0], px);
  lo[1] = fminf(lo[1], py); hi[1] = fmaxf(hi[1], py);
}

// false: the triangle gives nothing in this camera
__device__ bool tri_setup(const Cam& C, const float* __restrict__ vc, int i0, int i1, int i2, Tri& T) {
  float p[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { p[0][k] = vc[3 * (int64_t)i0 + k]; p[1][k] = vc[3 * (int64_t)i1 + k]; p[2][k] = vc[3 * (int64_t)i2 + k]; }
  const bool in0 = p[0][2] >= C.znear, in1 = p[1][2] >= C.znear, in2 = p[2][2] >= C.znear;
  if (!(in0 || in1 || in2)) return false;
  double a[3], b[3], c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { a[k] = p[0][k]; b[k] = p[1][k]; c[k] = p[2][k]; }
  cross64(b, c, T.n[0]);
  cross64(c, a, T.n[1]);
  cross64(a, b, T.n[2]);
  double det = (a[0] * T.n[0][0] + a[1] * T.n[0][1]) + a[2] * T.n[0][2];
  if (!(det < 0.0 || det > 0.0)) return false;
  if (det > 0.0) {
    if (C.cull) return false;
  } else {
    det = -det;
#pragma unroll
    for (int e = 0; e < 3; ++e)
#pragma unroll
      for (int k = 0; k < 3; ++k) T.n[e][k] = -T.n[e][k];
  }
  T.det = det;
  float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
  const bool in[3] = {in0, in1, in2};
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int f = (e + 1) % 3;
    if (in[e]) box_add(C, p[e][0], p[e][1], p[e][2], lo, hi);
    if (in[e] != in[f]) {
      const float s = (C.znear - p[e][2]) / (p[f][2] - p[e][2]);
      box_add(C, p[e][0] + s * (p[f][0] - p[e][0]), p[e][1] + s * (p[f][1] - p[e][1]), C.znear, lo, hi);
    }
  }
  // (a NaN bound becomes the image's: fmaxf / fminf return the other operand)
  const float fx0 = fmaxf(floorf(lo[0]) - 1.0f, 0.0f), fx1 = fminf(ceilf(hi[0]) + 1.0f, (float)(C.W - 1));
  const float fy0 = fmaxf(floorf(lo[1]) - 1.0f, 0.0f), fy1 = fminf(ceilf(hi[1]) + 1.0f, (float)(C.H - 1));
  if (!(fx1 >= fx0 && fy1 >= fy0)) return false;
  T.x0 = (int)fx0; T.x1 = (int)fx1; T.y0 = (int)fy0; T.y1 = (int)fy1;
  return true;
}

__device__ __forceinline__ bool covers(double e, const double n[3]) {
  return e > 0.0 || (e == 0.0 && (n[0] > 0.0 || (n[0] == 0.0 && n[1] > 0.0)));
}

__device__ __forceinline__ void sample(const Cam& C, const Tri& T, int u, int v, uint32_t* __restrict__ img) {
  const double dx = ((double)u - (double)C.cx) / (double)C.fx, dy = ((double)v - (double)C.cy) / (double)C.fy;
  const double e0 = (T.n[0][0] * dx + T.n[0][1] * dy) + T.n[0][2];
  const double e1 = (T.n[1][0] * dx + T.n[1][1] * dy) + T.n[1][2];
  const double e2 = (T.n[2][0] * dx + T.n[2][1] * dy) + T.n[2][2];
  if (!(covers(e0, T.n[0]) && covers(e1, T.n[1]) && covers(e2, T.n[2]))) return;
  const double s = (e0 + e1) + e2;
  if (!(s > 0.0)) return;
  const float z = (float)(T.det / s);
  if (!(z >= C.znear && z <= C.zfar)) return;
  atomicMin(&img[(int64_t)v * C.W + u], __float_as_uint(z));
}

__global__ __launch_bounds__(RS_THREADS) void rs_project(const float* __restrict__ verts, int64_t V, const float* __restrict__ w2c,
                                                         int cam0, float* __restrict__ vcam) {
  const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (i >= V) return;
  const float* w = w2c + 12 * (int64_t)(cam0 + blockIdx.y);
  const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
  float* o = vcam + 3 * ((int64_t)blockIdx.y * V + i);
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = ((w[4 * k] * x + w[4 * k + 1] * y) + w[4 * k + 2] * z) + w[4 * k + 3];
}

// counters (n_cam, 2): [0] triangles handed to rs_large, [1] triangles walked here
__global__ __launch_bounds__(RS_THREADS) void rs_small(Cam C, const float* __restrict__ vcam, int64_t V, const int32_t* __restrict__ faces,
                                                       int64_t F, int cam0, int32_t* __restrict__ list, int32_t* __restrict__ counters,
                                                       uint32_t* __restrict__ depth, int32_t* __restrict__ status) {
  const int64_t f = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  const int cl = blockIdx.y, cam = cam0 + cl;
  const float* vc = vcam + 3 * (int64_t)cl * V;
  uint32_t* img = depth + (int64_t)cam * C.H * C.W;
  Tri T;
  int kind = 0;                                  // 0 nothing, 1 walked here, 2 listed
  if (f < F) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) {
      *status = 1;
    } else if (tri_setup(C, vc, i0, i1, i2, T)) {
      const int64_t area = (int64_t)(T.x1 - T.x0 + 1) * (T.y1 - T.y0 + 1);
      kind = area <= I2SDF_RASTER_SMALL_MAX ? 1 : 2;
    }
  }
  if (kind == 1)
    for (int v = T.y0; v <= T.y1; ++v)
      for (int u = T.x0; u <= T.x1; ++u) sample(C, T, u, v, img);
  // wave-aggregated counters: one atomic per wave and kind
  const int lane = threadIdx.x & 63;
  const unsigned long long m1 = __ballot(kind == 1), m2 = __ballot(kind == 2);
  const int lead = __ffsll((long long)(m1 | m2)) - 1;
  int base = 0;
  if (lane == lead) {
    if (m1) atomicAdd(&counters[2 * cam + 1], __popcll(m1));
    if (m2) base = atomicAdd(&counters[2 * cam], __popcll(m2));
  }
  if (m2) {
    base = __shfl(base, lead, 64);
    if (kind == 2) list[(int64_t)cl * F + base + __popcll(m2 & ((1ull << lane) - 1ull))] = (int32_t)f;
  }
}

__global__ __launch_bounds__(RS_THREADS) void rs_large(Cam C, const float* __restrict__ vcam, int64_t V, const int32_t* __restrict__ faces,
                                                       int64_t F, int cam0, const int32_t* __restrict__ list,
                                                       const int32_t* __restrict__ counters, uint32_t* __restrict__ depth) {
  const int cl = blockIdx.y, cam = cam0 + cl;
  const float* vc = vcam + 3 * (int64_t)cl * V;
  uint32_t* img = depth + (int64_t)cam * C.H * C.W;
  const int n = counters[2 * cam];
  for (int it = blockIdx.x; it < n; it += gridDim.x) {
    const int64_t f = list[(int64_t)cl * F + it];
    Tri T;
    if (!tri_setup(C, vc, faces[3 * f], faces[3 * f + 1], faces[3 * f + 2], T)) continue;   // (uniform over the workgroup)
    const int bw = T.x1 - T.x0 + 1;
    const int64_t area = (int64_t)bw * (T.y1 - T.y0 + 1);
    for (int64_t q = threadIdx.x; q < area; q += RS_THREADS) sample(C, T, T.x0 + (int)(q % bw), T.y0 + (int)(q / bw), img);
  }
}

// no hit (the fill pattern) -> 0
__global__ __launch_bounds__(RS_THREADS) void rs_finish(uint32_t* __restrict__ depth, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (i < n && depth[i] == RS_EMPTY) depth[i] = 0u;
}

struct Plan {
  int64_t per_cam, bytes;
  int chunk;
  int64_t off_list;                              // (per chunk: vcam fp32 (chunk, V, 3), then list int32 (chunk, F))
};

int64_t align16(int64_t x) { return (x + 15) / 16 * 16; }

bool plan(int64_t V, int64_t F, int32_t n_cam, Plan& P) {
  if (V < 1 || F < 1 || n_cam < 1 || V > INT32_MAX || F > INT32_MAX || n_cam > 65535) return false;
  P.per_cam = align16(12 * V) + align16(4 * F);
  const int64_t all = P.per_cam * n_cam;
  P.bytes = all <= RS_BUDGET ? all : (P.per_cam > RS_BUDGET ? P.per_cam : RS_BUDGET);      // (monotone in V, F and n_cam)
  P.chunk = (int)(P.bytes / P.per_cam);
  P.off_list = align16(12 * V) * P.chunk;
  return true;
}

}  // namespace

extern "C" int64_t i2sdf_raster_workspace_bytes(int64_t n_verts, int64_t F, int32_t n_cam) {
  Plan P;
  return plan(n_verts, F, n_cam, P) ? P.bytes : 0;
}

extern "C" int i2sdf_raster_depth(const float* verts, int64_t n_verts, const int32_t* faces, int64_t F, const float* w2c, int32_t n_cam,
                                  const float* K4, int32_t H, int32_t W, float znear, float zfar, int32_t cull, void* workspace,
                                  float* depth, int32_t* counters, int32_t* status, void* stream) {
  if (n_verts < 0 || F < 0 || n_cam < 0 || n_verts > INT32_MAX || F > INT32_MAX || n_cam > 65535 || H < 1 || W < 1 || !K4) return I2SDF_EINVAL;
  if ((int64_t)H * W > INT32_MAX || (int64_t)H * W * n_cam > (int64_t)INT32_MAX * RS_THREADS || (cull != 0 && cull != 1)) return I2SDF_EINVAL;
  if (!(K4[0] > 0.0f && K4[1] > 0.0f && K4[0] < INFINITY && K4[1] < INFINITY && fabsf(K4[2]) < INFINITY && fabsf(K4[3]) < INFINITY))
    return I2SDF_EINVAL;
  if (!(znear > 0.0f && zfar >= znear && zfar < INFINITY)) return I2SDF_EINVAL;
  if (n_cam == 0) return I2SDF_OK;
  if (!depth || !counters || !status) return I2SDF_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_pix = (int64_t)n_cam * H * W;
  const bool empty = n_verts == 0 || F == 0;
  Plan P;
  if (!empty && (!verts || !faces || !w2c || !workspace || !plan(n_verts, F, n_cam, P))) return I2SDF_EINVAL;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(counters, 0, 8 * (size_t)n_cam, st), "raster counters")) return rc;
  if (int rc = i2sdf_hip_check(hipMemsetAsync(depth, empty ? 0 : 0xFF, 4 * (size_t)n_pix, st), "raster depth fill")) return rc;
  if (empty) return I2SDF_OK;
  const Cam C{K4[0], K4[1], K4[2], K4[3], znear, zfar, H, W, cull};
  float* vcam = (float*)workspace;
  int32_t* list = (int32_t*)((char*)workspace + P.off_list);
  const unsigned vb = (unsigned)((n_verts + RS_THREADS - 1) / RS_THREADS), fb = (unsigned)((F + RS_THREADS - 1) / RS_THREADS);
  const unsigned lb = (unsigned)(F < RS_LARGE_BLOCKS ? F : RS_LARGE_BLOCKS);
  for (int cam0 = 0; cam0 < n_cam; cam0 += P.chunk) {
    const unsigned nc = (unsigned)(n_cam - cam0 < P.chunk ? n_cam - cam0 : P.chunk);
    rs_project<<<dim3(vb, nc), RS_THREADS, 0, st>>>(verts, n_verts, w2c, cam0, vcam);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "rs_project")) return rc;
    rs_small<<<dim3(fb, nc), RS_THREADS, 0, st>>>(C, vcam, n_verts, faces, F, cam0, list, counters, (uint32_t*)depth, status);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "rs_small")) return rc;
    rs_large<<<dim3(lb, nc), RS_THREADS, 0, st>>>(C, vcam, n_verts, faces, F, cam0, list, counters, (uint32_t*)depth);
    if (int rc = i2sdf_hip_check(hipGetLastError(), "rs_large")) return rc;
  }
  rs_finish<<<(unsigned)((n_pix + RS_THREADS - 1) / RS_THREADS), RS_THREADS, 0, st>>>((uint32_t*)depth, n_pix);
  return i2sdf_hip_check(hipGetLastError(), "rs_finish");
}
