// Host build of csrc/tri_closest.h for tests/test_closest_host.py: reads records of one point and one face, writes what tri_closest,
// tri_degenerate, box_dist2 (on the face's own exact box, the tightest the tree can hold) and box_skip_above (for that face's own
// computed d2) say.
//   in : int32 n, then n x 12 fp32: p[3], A[3], B[3], C[3]
//   out: n x 11 fp64: c[3], d2, u, v, feature, degenerate, q, skip_above, skipped
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../i2sdf_amd/csrc/tri_closest.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 3;
  int32_t n = 0;
  if (fread(&n, 4, 1, in) != 1 || n < 0) return 4;
  std::vector<float> rec((size_t)n * 12);
  if (fread(rec.data(), 4, rec.size(), in) != rec.size()) return 5;
  for (int32_t i = 0; i < n; ++i) {
    const float* q = rec.data() + (size_t)i * 12;
    i2sdf::ClosestHit h;
    i2sdf::tri_closest(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], h);
    float lo[3], hi[3];
    double M = 0.0;
    for (int k = 0; k < 3; ++k) {
      const float a = q[3 + k], b = q[6 + k], c = q[9 + k];
      lo[k] = a; if (b < lo[k]) lo[k] = b; if (c < lo[k]) lo[k] = c;
      hi[k] = a; if (b > hi[k]) hi[k] = b; if (c > hi[k]) hi[k] = c;
      M = fmax(M, fmax(fabs((double)q[k]), fmax(fabs((double)lo[k]), fabs((double)hi[k]))));
    }
    double res[11] = {h.c0, h.c1, h.c2, h.d2, h.u, h.v, (double)h.feature, 0.0, 0.0, 0.0, 0.0};
    res[7] = i2sdf::tri_degenerate(q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11]);
    res[8] = i2sdf::box_dist2(q[0], q[1], q[2], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    res[9] = i2sdf::box_skip_above(h.d2, M);
    res[10] = res[8] > res[9];
    fwrite(res, 8, 11, out);
  }
  fclose(in);
  fclose(out);
  return 0;
}
