// Host build of csrc/quadric.h for tests/test_simplify_host.py: reads the corner runs of cells, adds their face quadrics in the order of
// include/i2sdf.h ("Mesh simplification": position j of a run in lane j mod 64, then the xor butterfly) and solves.
//   in : int32 n_cells, fp64 reg, fp64 h, then per cell: int32 n_corners, 3 fp64 cc, 3 fp64 m, n_corners x 9 fp32 (a, b, c)
//   out: n_cells x 13 fp64: A (6), bvec (3), x (3), fallback
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../i2sdf_amd/csrc/quadric.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 3;
  int32_t n = 0;
  double reg = 0.0, h = 0.0;
  if (fread(&n, 4, 1, in) != 1 || n < 0 || fread(&reg, 8, 1, in) != 1 || fread(&h, 8, 1, in) != 1) return 4;
  for (int32_t i = 0; i < n; ++i) {
    int32_t k = 0;
    double cc[3], m[3];
    if (fread(&k, 4, 1, in) != 1 || k < 0 || fread(cc, 8, 3, in) != 3 || fread(m, 8, 3, in) != 3) return 5;
    std::vector<float> rec((size_t)k * 9);
    if (fread(rec.data(), 4, rec.size(), in) != rec.size()) return 6;
    double part[64][i2sdf::QD_VALUES] = {};
    for (int32_t j = 0; j < k; ++j) {
      const float* r = rec.data() + (size_t)j * 9;
      const double a[3] = {r[0], r[1], r[2]}, b[3] = {r[3], r[4], r[5]}, c[3] = {r[6], r[7], r[8]};
      double q[i2sdf::QD_VALUES];
      i2sdf::quadric_face(a, b, c, cc, q);
      for (int v = 0; v < i2sdf::QD_VALUES; ++v) part[j % 64][v] += q[v];
    }
    for (int s = 32; s > 0; s >>= 1) {
      double next[64][i2sdf::QD_VALUES];
      for (int l = 0; l < 64; ++l)
        for (int v = 0; v < i2sdf::QD_VALUES; ++v) next[l][v] = part[l][v] + part[l ^ s][v];
      for (int l = 0; l < 64; ++l)
        for (int v = 0; v < i2sdf::QD_VALUES; ++v) part[l][v] = next[l][v];
    }
    double res[13];
    for (int v = 0; v < i2sdf::QD_VALUES; ++v) res[v] = part[0][v];
    res[12] = i2sdf::quadric_solve(part[0], reg, m, 0.5 * h, res + 9) ? 1.0 : 0.0;
    fwrite(res, 8, 13, out);
  }
  fclose(in);
  fclose(out);
  return 0;
}
