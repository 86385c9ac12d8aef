// Host-only probe of the weight-gradient launch plan (tests/test_wgrad_plan.py): reads a binary i2sdf_net_desc, creates the plan (no GPU
// needed), sets the options given as `option=value` and prints what i2sdf_weight_grads would enqueue for a batch of M_sdf / M_main points:
//   every pass in order -- kernel, threads, LDS bytes, main or side stream -- its WgLaunch batches, every WgTask and WgJob field of every task;
//   the table of the final reduction (wn_backward_kernel), every WnLayer field.
// Operand pointers are printed as <buffer>+<floats> from fake bases, nothing is dereferenced.  The passes are those of the ranged shape
// when the plan has point ranges (I2SDF_OPT_PARTS), else those of the fork / join shape.
//   wgrad_probe net.desc M_sdf M_main with_fbar [option=value ...]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "wgrad_plan.h"
using namespace i2sdf;

static const char* const BUF[] = {"pe", "hs", "abars", "gus", "gpbar", "gas", "ga_last4", "ones4", "fbar", "pev", "feat", "rs", "gar", "ga_last_rgb",
                                  "hl", "gal0", "gal_last"};
constexpr int N_BUF = sizeof(BUF) / sizeof(BUF[0]);
static const float* base(int i) { return reinterpret_cast<const float*>(uintptr_t(i + 1) << 40); }      // never dereferenced

static void show_ptr(const float* q) {
  if (!q) { printf(" null"); return; }
  const int i = (int)(reinterpret_cast<uintptr_t>(q) >> 40) - 1;
  if (i < 0 || i >= N_BUF) { printf(" ?"); return; }
  printf(" %s+%lld", BUF[i], (long long)(q - base(i)));
}

int main(int argc, char** argv) {
  i2sdf_net_desc desc;
  FILE* f = argc > 4 ? fopen(argv[1], "rb") : nullptr;
  if (!f || fread(&desc, sizeof(desc), 1, f) != 1) return 2;
  fclose(f);
  i2sdf_plan* p = nullptr;
  if (i2sdf_plan_create(&desc, &p) != I2SDF_OK) return 3;
  for (int i = 5; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq || i2sdf_plan_set_option(p, atoi(argv[i]), atoi(eq + 1)) != I2SDF_OK) return 4;
  }
  i2sdf_train_buffers tb{};
  tb.M_sdf = atoll(argv[2]); tb.M_main = atoll(argv[3]); tb.Mp = (tb.M_sdf + 127) / 128 * 128;
  const float** slot[N_BUF] = {&tb.pe, &tb.hs, &tb.abars, &tb.gus, &tb.gpbar, &tb.gas, &tb.ga_last4, &tb.ones4, &tb.fbar, &tb.pev, &tb.feat, &tb.rs,
                               &tb.gar, &tb.ga_last_rgb, &tb.hl, &tb.gal0, &tb.gal_last};
  for (int i = 0; i < N_BUF; ++i) *slot[i] = base(i);
  if (!atoi(argv[4])) tb.fbar = nullptr;
  if (p->light.d.n_lin == 0) tb.hl = tb.gal0 = tb.gal_last = nullptr;
  float* const partials = const_cast<float*>(base(N_BUF - 1)) + (int64_t(1) << 36);      // (prints as gal_last+2^36)

  static const char* const KERN[WGK_COUNT] = {"wgrad_all_kernel<2>", "wgrad_all_kernel<3>", "wgrad3p_kernel<2>", "wgrad3p_kernel<3>",
                                              "wgrad_kernel<0,0>", "wgrad_narrow_kernel<3>", "wgrad_narrow_kernel<0>"};
  const std::vector<WgPass> passes = wgrad_passes(p, &tb, partials, i2sdf_parts_on(p));
  for (const WgPass& ps : passes) {
    printf("pass %s threads %d lds %d stream %s batches %d\n", KERN[ps.kern], ps.threads, ps.lds_bytes, ps.side ? "side" : "main", (int)ps.batches.size());
    for (const WgLaunch& L : ps.batches) {
      printf("batch %d %d %lld", L.n, L.chunk0, (long long)L.chunk_stride);
      show_ptr(L.partials);
      printf("\n");
      for (int i = 0; i < L.n; ++i) {
        const WgTask& t = L.t[i];
        printf("task %d %d %d %d %d %d %d %d %lld %lld\n", t.variant, t.njobs, t.relu_b, t.has_bias, t.rows_store, t.cols_store, t.ldo, t.pad,
               (long long)t.out_off, (long long)t.bias_off);
        for (int jb = 0; jb < t.njobs; ++jb) {
          const WgJob& j = t.j[jb];
          printf("job");
          show_ptr(j.A);
          show_ptr(j.B);
          printf(" %d %d %d %d %lld %lld %lld %d %d %d %d\n", j.lda, j.ldb, j.a_w, j.b_w, (long long)j.m_count, (long long)j.a_blk, (long long)j.b_blk,
                 j.a_c0, j.b_c0, j.a_p24, j.b_p24);
        }
      }
    }
  }
  const WnTab tab = wgrad_wn_tab(p, &tb);
  printf("wn %d %d\n", tab.n, tab.n_rows);
  for (int i = 0; i < tab.n; ++i) {
    const WnLayer& y = tab.l[i];
    uint32_t mb;
    memcpy(&mb, &y.mult, 4);
    printf("wnlayer %lld %lld %lld %lld %lld %d %d %d %d %d %d %d %d %d %08x\n", (long long)y.off_v, (long long)y.off_g, (long long)y.off_bias,
           (long long)y.blk_off, (long long)y.bias_blk_off, y.rows, y.cols, y.row0, y.ldo, y.rsplit, y.rbase, y.split, y.base1, y.valid0, mb);
  }
  i2sdf_plan_destroy(p);
  return 0;
}
