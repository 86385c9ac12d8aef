// Host build of csrc/tri_solid_angle.h for tests/test_winding_host.py: reads records of one point and one face, writes what
// tri_solid_angle_terms and tri_solid_angle say, the face's raw moments about o, the record wn_finish makes of them with the face's
// own exact box, and what wn_far_field says of that record at beta = 2.
//   in : int32 n, 3 fp64 o, then n x 12 fp32: q[3], A[3], B[3], C[3]
//   out: n x 37 fp64: det, den, omega, m[16], t[16], accepted, far-field omega (0 when not accepted)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../i2sdf_amd/csrc/tri_solid_angle.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 3;
  int32_t n = 0;
  double o[3];
  if (fread(&n, 4, 1, in) != 1 || n < 0 || fread(o, 8, 3, in) != 3) return 4;
  std::vector<float> rec((size_t)n * 12);
  if (fread(rec.data(), 4, rec.size(), in) != rec.size()) return 5;
  for (int32_t i = 0; i < n; ++i) {
    const float* q = rec.data() + (size_t)i * 12;
    double res[37] = {0.0};
    i2sdf::tri_solid_angle_terms(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], res[0], res[1]);
    res[2] = i2sdf::tri_solid_angle(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11]);
    i2sdf::tri_moments(q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], o[0], o[1], o[2], res + 3);
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
      const float a = q[3 + k], b = q[6 + k], c = q[9 + k];
      lo[k] = a; if (b < lo[k]) lo[k] = b; if (c < lo[k]) lo[k] = c;
      hi[k] = a; if (b > hi[k]) hi[k] = b; if (c > hi[k]) hi[k] = c;
    }
    i2sdf::wn_finish(res + 3, o[0], o[1], o[2], lo, hi, res + 19);
    double omega = 0.0;
    res[35] = i2sdf::wn_far_field(q[0], q[1], q[2], res + 19, 4.0, omega) ? 1.0 : 0.0;
    res[36] = omega;
    fwrite(res, 8, 37, out);
  }
  fclose(in);
  fclose(out);
  return 0;
}
