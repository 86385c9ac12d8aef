// Host build of csrc/tri_isect.h for tests/test_raycast_host.py: reads records of one ray, one face and bounds, writes what tri_hit and
// box_may_hit (on the face's own exact box, the tightest the tree can hold) say.
//   in : int32 n, then n x 18 fp32: o[3], d[3], A[3], B[3], C[3], t_min, t_max, cull
//   out: n x (int32 ray_ok, int32 accept, int32 box, fp32 t, u, v)
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../i2sdf_amd/csrc/tri_isect.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 3;
  int32_t n = 0;
  if (fread(&n, 4, 1, in) != 1 || n < 0) return 4;
  std::vector<float> rec((size_t)n * 18);
  if (fread(rec.data(), 4, rec.size(), in) != rec.size()) return 5;
  for (int32_t i = 0; i < n; ++i) {
    const float* q = rec.data() + (size_t)i * 18;
    i2sdf::RayShear r;
    int32_t flags[3] = {0, 0, 0};
    float res[3] = {0.0f, 0.0f, 0.0f};
    flags[0] = i2sdf::ray_shear(q[0], q[1], q[2], q[3], q[4], q[5], r);
    if (flags[0]) {
      flags[1] = i2sdf::tri_hit(r, q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13], q[14], q[15], q[16], (int)q[17], res[0], res[1], res[2]);
      float lo[3], hi[3], t_near;
      for (int k = 0; k < 3; ++k) {
        const float a = q[6 + k], b = q[9 + k], c = q[12 + k];
        lo[k] = a; if (b < lo[k]) lo[k] = b; if (c < lo[k]) lo[k] = c;
        hi[k] = a; if (b > hi[k]) hi[k] = b; if (c > hi[k]) hi[k] = c;
      }
      flags[2] = i2sdf::box_may_hit(r, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], q[15], q[16], t_near);
    }
    if (!flags[1]) res[0] = res[1] = res[2] = 0.0f;
    fwrite(flags, 4, 3, out);
    fwrite(res, 4, 3, out);
  }
  fclose(in);
  fclose(out);
  return 0;
}
