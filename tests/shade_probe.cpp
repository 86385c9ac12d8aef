// Host-only probe of csrc/brdf_dev.h (tests/test_shade_host.py): the per-sample function the shading kernels run, compiled for the CPU.
//   shade_probe <raw file> <bn> <spp> <f32|f64>
// The raw file holds fp32 arrays back to back: normal (bn,3), view (bn,3), Kd (bn,3), Ks (bn,3), rough (bn), samples (bn,spp,3).  One line
// per (point, sample): wo (3, local), pdf, f_spec (3), then d / d rough of the same seven, evaluated in the precision asked for.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "brdf_dev.h"
using namespace i2sdf_brdf;

template <class T>
static void run(const std::vector<float>& in, long bn, long spp) {
  const float *normal = in.data(), *view = normal + 3 * bn, *Kd = view + 3 * bn, *Ks = Kd + 3 * bn, *rough = Ks + 3 * bn, *samples = rough + bn;
  for (long p = 0; p < bn; ++p) {
    const T n[3] = {T(normal[3 * p]), T(normal[3 * p + 1]), T(normal[3 * p + 2])};
    const T v[3] = {T(view[3 * p]), T(view[3 * p + 1]), T(view[3 * p + 2])};
    const T kd[3] = {T(Kd[3 * p]), T(Kd[3 * p + 1]), T(Kd[3 * p + 2])};
    const T ks[3] = {T(Ks[3 * p]), T(Ks[3 * p + 1]), T(Ks[3 * p + 2])};
    Point<T> pt;
    point_setup(n, v, kd, ks, pt);
    for (long s = 0; s < spp; ++s) {
      const float* u = samples + 3 * (p * spp + s);
      Sample<Dual<T>> o;
      sample_eval(pt, Dual<T>{T(rough[p]), T(1)}, T(u[0]), T(u[1]), T(u[2]), o);
      Dual<T> row[7] = {o.wo[0], o.wo[1], o.wo[2], o.pdf, spec_channel(pt, o, 0), spec_channel(pt, o, 1), spec_channel(pt, o, 2)};
      for (int k = 0; k < 7; ++k) printf("%.17g ", (double)row[k].v);
      for (int k = 0; k < 7; ++k) printf("%.17g%c", (double)row[k].d, k == 6 ? '\n' : ' ');
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const long bn = atol(argv[2]), spp = atol(argv[3]);
  if (bn < 1 || spp < 1) return 2;
  std::vector<float> in((size_t)(13 * bn + 3 * bn * spp));
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(in.data(), sizeof(float), in.size(), f) != in.size()) return 3;
  fclose(f);
  if (!strcmp(argv[4], "f32")) run<float>(in, bn, spp);
  else if (!strcmp(argv[4], "f64")) run<double>(in, bn, spp);
  else return 2;
  return 0;
}
