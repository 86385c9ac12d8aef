// Host-only probe of the plan (tests/test_plan_spans.py): reads a binary i2sdf_net_desc, creates the plan (no GPU needed) and prints
//   the segment table, every Seg field, one line per segment;
//   for every launch site's span: the chunk its stream starts at and the number of stages it walks, or "refused";
//   what span() answers to an empty span and to one that is not a whole number of stages.
#include <stdio.h>
#include <string.h>
#include "plan.h"
using namespace i2sdf;

static const float* const PACKED = reinterpret_cast<const float*>(uintptr_t(1) << 32);      // never dereferenced

static void show(const char* name, const i2sdf_plan* p, const NetPlan& np, SpanId id) {
  const Span s = span(p, PACKED, np, id);
  if (s.n_stages) printf("span %s %lld %d\n", name, (long long)((s.w - PACKED - p->scale_floats) / CHUNK_FLOATS), s.n_stages);
  else printf("span %s refused\n", name);
}

int main(int argc, char** argv) {
  i2sdf_net_desc desc;
  FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
  if (!f || fread(&desc, sizeof(desc), 1, f) != 1) return 2;
  fclose(f);
  i2sdf_plan* p = nullptr;
  if (i2sdf_plan_create(&desc, &p) != I2SDF_OK) {
    fprintf(stderr, "i2sdf_plan_create refused: %s\n", i2sdf_last_hip_error());      // (tests/test_shape_frontier.py reads the reason)
    return 3;
  }
  printf("segs %d total_chunks %lld scale_floats %lld\n", p->n_segs, (long long)p->total_chunks, (long long)p->scale_floats);
  for (const Seg& s : p->segs) {
    uint32_t mb;
    memcpy(&mb, &s.mult, 4);
    printf("seg %lld %d %d %lld %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %08x\n", (long long)s.chunk0, s.nchunks, s.type, (long long)s.off_v,
           (long long)s.off_bias, s.scale_off, s.rows, s.cols, s.row_off, s.nrows, s.NT, s.KC, s.used, s.cm.split, s.cm.base0, s.cm.valid0, s.cm.base1,
           s.cm.valid1, mb);
  }
  show("sdf.fwd_hidden", p, p->sdf, SPAN_FWD_HIDDEN);        // i2sdf_sdf_backward, sweep 1
  show("sdf.fwd_sdf", p, p->sdf, SPAN_FWD_SDF);              // launch_sdf_fwd / i2sdf_sdf_forward_grad without features
  show("sdf.fwd_all", p, p->sdf, SPAN_FWD);                  // ... with features
  show("sdf.rev_sweep2", p, p->sdf, SPAN_REV_SWEEP2);        // i2sdf_sdf_backward, sweep 2
  show("sdf.rev_chain", p, p->sdf, SPAN_REV_CHAIN);          // i2sdf_sdf_forward_grad, d sdf/dx chain
  show("sdf.fwd3_hidden", p, p->sdf, SPAN_FWD3_HIDDEN);
  show("sdf.fwd3_all", p, p->sdf, SPAN_FWD3);
  show("sdf.rev3_sweep2", p, p->sdf, SPAN_REV3_SWEEP2);
  show("sdf.rev3_chain", p, p->sdf, SPAN_REV3_CHAIN);
  show("sdf.fwd3h_sdf", p, p->sdf, SPAN_FWD3H_SDF);
  show("sdf.fwd3h_all", p, p->sdf, SPAN_FWD3H);
  show("sdf.fwd2h", p, p->sdf, SPAN_FWD2H);
  show("rgb.fwd", p, p->rgb, SPAN_FWD);
  show("rgb.rev", p, p->rgb, SPAN_REV);
  show("rgb.fwd3h", p, p->rgb, SPAN_FWD3H);
  show("rgb.rev3h", p, p->rgb, SPAN_REV3H);
  if (p->light.d.n_lin > 0) {
    show("light.fwd", p, p->light, SPAN_FWD);
    show("light.rev", p, p->light, SPAN_REV);
    show("light.fwd3h", p, p->light, SPAN_FWD3H);
  }
  // behind the recorded part of the output: the refusals
  const int64_t whole = span_chunks(p->sdf, SPAN_FWD);
  printf("check empty %d\n", span(p, PACKED, p->sdf, SpanId{FWD, FWD, SC}).n_stages);
  printf("check backwards %d\n", span(p, PACKED, p->sdf, SpanId{FWD_END, FWD, SC}).n_stages);
  printf("check ragged %d\n", span(p, PACKED, p->sdf, SpanId{FWD, FWD_END, (int)whole - 1}).n_stages);
  printf("check whole %d\n", span(p, PACKED, p->sdf, SpanId{FWD, FWD_END, (int)whole}).n_stages);
  i2sdf_plan_destroy(p);
  return 0;
}
