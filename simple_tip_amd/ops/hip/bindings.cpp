// Python bindings for the simple_tip_amd HIP/CDNA4 kernels (gfx950).
//
// Native HIP throughout — no CUDA-compat paths; streams come from torch's
// HIP stream pool so kernels serialize correctly with torch ops.

#include <torch/extension.h>

#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "cam_many.h"
#include "coverage_suite.h"
#include "kmeans_many.h"

// launchers defined in the .hip translation units
void launch_rownorm(const float*, int, int, float*, hipStream_t);
void launch_pairwise_full(const float*, const float*, const float*,
                          const float*, int, int, int, float*, hipStream_t);
void launch_pairwise_rowmin(const float*, const float*, const float*,
                            const float*, int, int, int, float*, int*, float*,
                            int64_t*, hipStream_t);
void launch_pairwise_kde(const float*, const float*, const float*,
                         const float*, int, int, int, float2*, float*,
                         hipStream_t);
void launch_grouped_rowmin(const float*, const float*, const float*,
                           const float*, const int*, const int*, int, int,
                           int, int, float*, int*, float*, int64_t*,
                           hipStream_t);
void launch_grouped_kde(const float*, const float*, const float*,
                        const float*, const int*, const int*, int, int, int,
                        int, float2*, float*, hipStream_t);
void launch_grouped_rowmin_bf16(const short*, const short*, const float*,
                                const float*, const int*, const int*, int,
                                int, int, int, float*, int*, float*,
                                int64_t*, hipStream_t);
void launch_grouped_kde_bf16(const short*, const short*, const float*,
                             const float*, const int*, const int*, int, int,
                             int, int, float2*, float*, hipStream_t);
// bf16 row-min dispatch (pairwise.hip): force the generic kernel, count the
// launches that took the pipelined one, and the pipelined kernel's geometry
void rowmin_bf16_force_generic(bool);
int64_t rowmin_bf16_pipelined_launches();
int rowmin_bf16_pipeline_bk();
int rowmin_bf16_pipeline_nbuf();
void launch_profile(int, const float*, const unsigned char*, const float*,
                    const float*, float, int, int, int, int,
                    unsigned long long*, long long*, hipStream_t);
void launch_popcount(const unsigned long long*, int, int, long long*,
                     hipStream_t);
void launch_tknc(const float*, int, int, int, int, int, unsigned long long*,
                 hipStream_t);
void launch_bucketize(const double*, const double*, int, int, int,
                      unsigned long long*, hipStream_t);
void launch_cam_greedy_coop(const unsigned long long*, int, int,
                            unsigned long long, unsigned char*,
                            unsigned long long*, long long*, int*, long long*,
                            int*, int*, int*, hipStream_t);
void launch_softmax_scores(const float*, int, int, float*, float*, float*,
                           float*, hipStream_t);
void launch_mfma_probe(const short*, const short*, float*, hipStream_t);
void launch_resblock(int, int, const short*, short*, const short*,
                     const float*, const short*, const float*, hipStream_t);
void launch_downblock(int, int, const short*, short*, const short*,
                      const float*, const short*, const float*, const short*,
                      const float*, hipStream_t);
void launch_stem(int, const short*, short*, const short*, const float*,
                 hipStream_t);
void launch_stage1(int, const float*, short*, const void* const*, hipStream_t);
void launch_stage2(int, const short*, short*, const void* const*, hipStream_t);
void launch_stage3(int, const short*, short*, float*, const void* const*,
                   hipStream_t);
void launch_mc_dropout_votes(const float*, const float*, const float*, int,
                             int, int, int, uint32_t, float, uint32_t,
                             uint32_t, uint32_t, int*, hipStream_t);
void launch_mc_dropout_stats(const float*, const float*, const float*, int,
                             int, int, int, uint32_t, float, uint32_t,
                             uint32_t, uint32_t, int*, float*, float*,
                             hipStream_t);
int segment_plan_max_classes();
void launch_segment_plan(const int64_t*, int, int, int, int*, int*, int*,
                         hipStream_t);
void launch_rownorm_bf16(const short*, int, int, const int*, float*,
                         hipStream_t);
int grouped_whiten_max_features();
void launch_grouped_whiten_bf16(const short*, int, int, const int*, const int*,
                                const int*, int, const int*, const short*, int,
                                int, int, int, short*, hipStream_t);
void launch_grouped_rowmin_plan(const short*, int, const short*, const float*,
                                const float*, const int*, const int*,
                                const int*, const float*, int, int, int, int,
                                float*, int*, float*, float*, int*,
                                hipStream_t);
void launch_grouped_kde_plan(const short*, const short*, const float*,
                             const float*, const int*, const int*, const int*,
                             int, const int*, const float*, int, int, int, int,
                             float2*, float*, hipStream_t);
void launch_grouped_center(const void*, bool, int, int, const int*, const int*,
                           const int*, int, int, const float*, int, float*,
                           hipStream_t);
int grouped_gauss_max_slots();
void launch_grouped_gauss_plan(const float*, const float*, const int*,
                               const int*, const int*, int, const float*, int,
                               int, int, int, float*, float*, hipStream_t);
int mc_dropout_max_grid(int, int);
int mc_dropout_rows_per_block();
int mc_dropout_max_classes();
int mc_dropout_max_features();
void launch_mc_transformer(const float*, const float*, const float* const*,
                           float, const uint32_t*, const float*, int, int, int,
                           int, int, int, uint32_t, uint32_t, uint32_t, int*,
                           float*, float*, bool, hipStream_t);
int mc_transformer_max_grid(int, int, int);
int mc_transformer_lds_bytes(int, int, int);
void mc_transformer_limits(int*);

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_f32_2d(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.dtype() == torch::kFloat32, name, " must be fp32");
  TORCH_CHECK(t.dim() == 2 && t.is_contiguous(), name,
              " must be 2D contiguous");
}

constexpr int kBN = 128;  // pairwise kernel column-block (matches pairwise.hip)

torch::Tensor rownorm(torch::Tensor x) {
  check_f32_2d(x, "x");
  auto out = torch::empty({x.size(0)}, x.options());
  launch_rownorm(x.data_ptr<float>(), x.size(0), x.size(1),
                 out.data_ptr<float>(), cur_stream());
  return out;
}

torch::Tensor pairwise_sqdist(torch::Tensor a, torch::Tensor b) {
  check_f32_2d(a, "a");
  check_f32_2d(b, "b");
  TORCH_CHECK(a.size(1) == b.size(1), "feature dims differ");
  const int m = a.size(0), n = b.size(0), k = a.size(1);
  auto an = rownorm(a);
  auto bn = rownorm(b);
  auto out = torch::empty({m, n}, a.options());
  launch_pairwise_full(a.data_ptr<float>(), b.data_ptr<float>(),
                       an.data_ptr<float>(), bn.data_ptr<float>(), m, n, k,
                       out.data_ptr<float>(), cur_stream());
  return out;
}

std::vector<torch::Tensor> rowmin_l2(torch::Tensor a, torch::Tensor b,
                                     c10::optional<torch::Tensor> bnorm) {
  check_f32_2d(a, "a");
  check_f32_2d(b, "b");
  TORCH_CHECK(a.size(1) == b.size(1), "feature dims differ");
  TORCH_CHECK(b.size(0) > 0, "rowmin_l2 against empty set");
  const int m = a.size(0), n = b.size(0), k = a.size(1);
  const int jb = (n + kBN - 1) / kBN;
  auto an = rownorm(a);
  auto bn = bnorm.has_value() ? bnorm.value() : rownorm(b);
  auto pval = torch::empty({jb, m}, a.options());
  auto pidx = torch::empty({jb, m}, a.options().dtype(torch::kInt32));
  auto dist = torch::empty({m}, a.options());
  auto idx = torch::empty({m}, a.options().dtype(torch::kInt64));
  launch_pairwise_rowmin(a.data_ptr<float>(), b.data_ptr<float>(),
                         an.data_ptr<float>(), bn.data_ptr<float>(), m, n, k,
                         pval.data_ptr<float>(), pidx.data_ptr<int>(),
                         dist.data_ptr<float>(), idx.data_ptr<int64_t>(),
                         cur_stream());
  return {dist, idx};
}

std::vector<torch::Tensor> grouped_rowmin(
    torch::Tensor testS, torch::Tensor trainS, torch::Tensor tseg,
    torch::Tensor nseg, torch::Tensor bnorm, int64_t jb_max) {
  check_f32_2d(testS, "testS");
  check_f32_2d(trainS, "trainS");
  TORCH_CHECK(tseg.is_cuda() && tseg.dtype() == torch::kInt32);
  TORCH_CHECK(nseg.is_cuda() && nseg.dtype() == torch::kInt32);
  const int bp = testS.size(0), k = testS.size(1);
  const int nclasses = tseg.size(0) - 1;
  auto an = rownorm(testS);
  auto pval = torch::empty({jb_max, bp}, testS.options());
  auto pidx = torch::empty({jb_max, bp}, testS.options().dtype(torch::kInt32));
  auto dist = torch::empty({bp}, testS.options());
  auto idx = torch::empty({bp}, testS.options().dtype(torch::kInt64));
  launch_grouped_rowmin(
      testS.data_ptr<float>(), trainS.data_ptr<float>(), an.data_ptr<float>(),
      bnorm.data_ptr<float>(), tseg.data_ptr<int>(), nseg.data_ptr<int>(),
      nclasses, bp, k, jb_max, pval.data_ptr<float>(), pidx.data_ptr<int>(),
      dist.data_ptr<float>(), idx.data_ptr<int64_t>(), cur_stream());
  return {dist, idx};
}

torch::Tensor grouped_kde(torch::Tensor testWS, torch::Tensor trainWS,
                          torch::Tensor tseg, torch::Tensor nseg,
                          torch::Tensor bnorm, int64_t jb_max) {
  check_f32_2d(testWS, "testWS");
  check_f32_2d(trainWS, "trainWS");
  const int bp = testWS.size(0), k = testWS.size(1);
  const int nclasses = tseg.size(0) - 1;
  auto an = rownorm(testWS);
  auto pkde = torch::empty({jb_max, bp, 2}, testWS.options());
  auto out = torch::empty({bp}, testWS.options());
  launch_grouped_kde(
      testWS.data_ptr<float>(), trainWS.data_ptr<float>(),
      an.data_ptr<float>(), bnorm.data_ptr<float>(), tseg.data_ptr<int>(),
      nseg.data_ptr<int>(), nclasses, bp, k, jb_max,
      reinterpret_cast<float2*>(pkde.data_ptr<float>()),
      out.data_ptr<float>(), cur_stream());
  return out;
}

std::vector<torch::Tensor> grouped_rowmin_bf16(
    torch::Tensor testS, torch::Tensor trainS, torch::Tensor tseg,
    torch::Tensor nseg, torch::Tensor anorm, torch::Tensor bnorm,
    int64_t jb_max) {
  TORCH_CHECK(testS.is_cuda() && testS.dtype() == torch::kBFloat16 &&
              testS.is_contiguous());
  TORCH_CHECK(trainS.dtype() == torch::kBFloat16 && trainS.is_contiguous());
  const int bp = testS.size(0), k = testS.size(1);
  const int nclasses = tseg.size(0) - 1;
  auto fopts = anorm.options();
  auto pval = torch::empty({jb_max, bp}, fopts);
  auto pidx = torch::empty({jb_max, bp}, fopts.dtype(torch::kInt32));
  auto dist = torch::empty({bp}, fopts);
  auto idx = torch::empty({bp}, fopts.dtype(torch::kInt64));
  launch_grouped_rowmin_bf16(
      reinterpret_cast<const short*>(testS.data_ptr()),
      reinterpret_cast<const short*>(trainS.data_ptr()),
      anorm.data_ptr<float>(), bnorm.data_ptr<float>(), tseg.data_ptr<int>(),
      nseg.data_ptr<int>(), nclasses, bp, k, jb_max, pval.data_ptr<float>(),
      pidx.data_ptr<int>(), dist.data_ptr<float>(), idx.data_ptr<int64_t>(),
      cur_stream());
  return {dist, idx};
}

torch::Tensor grouped_kde_bf16(torch::Tensor testWS, torch::Tensor trainWS,
                               torch::Tensor tseg, torch::Tensor nseg,
                               torch::Tensor anorm, torch::Tensor bnorm,
                               int64_t jb_max) {
  TORCH_CHECK(testWS.is_cuda() && testWS.dtype() == torch::kBFloat16 &&
              testWS.is_contiguous());
  TORCH_CHECK(trainWS.dtype() == torch::kBFloat16 && trainWS.is_contiguous());
  const int bp = testWS.size(0), k = testWS.size(1);
  const int nclasses = tseg.size(0) - 1;
  auto fopts = anorm.options();
  auto pkde = torch::empty({jb_max, bp, 2}, fopts);
  auto out = torch::empty({bp}, fopts);
  launch_grouped_kde_bf16(
      reinterpret_cast<const short*>(testWS.data_ptr()),
      reinterpret_cast<const short*>(trainWS.data_ptr()),
      anorm.data_ptr<float>(), bnorm.data_ptr<float>(), tseg.data_ptr<int>(),
      nseg.data_ptr<int>(), nclasses, bp, k, jb_max,
      reinterpret_cast<float2*>(pkde.data_ptr<float>()),
      out.data_ptr<float>(), cur_stream());
  return out;
}

// ---- sync-free grouped scoring (segment plan + gathered kernels) ----
// Every function below writes into caller-owned workspaces and enqueues on
// the current stream only: no allocation-dependent sizes, no host copies.

int64_t segment_plan_rows(int64_t b, int64_t c) {
  return 128 * ((b + 127) / 128 + c);
}

void check_dev(const torch::Tensor& t, torch::ScalarType dt, int64_t numel,
               const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name,
              " must be a contiguous GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " has the wrong dtype");
  TORCH_CHECK(t.numel() == numel, name, " has ", t.numel(),
              " elements, expected ", numel);
}

const short* bf16_ptr(const torch::Tensor& t);  // defined below

void segment_plan_out(torch::Tensor pred, int64_t nclasses, torch::Tensor tseg,
                      torch::Tensor rowmap, torch::Tensor dest) {
  TORCH_CHECK(pred.dim() == 1, "pred must be 1D");
  TORCH_CHECK(nclasses >= 1 && nclasses <= segment_plan_max_classes(),
              "segment_plan supports 1..", segment_plan_max_classes(),
              " classes");
  const int64_t b = pred.size(0);
  TORCH_CHECK(b >= 1 && b < (1 << 30), "bad batch size");
  check_dev(pred, torch::kInt64, b, "pred");
  check_dev(tseg, torch::kInt32, nclasses + 1, "tseg");
  check_dev(rowmap, torch::kInt32, segment_plan_rows(b, nclasses), "rowmap");
  check_dev(dest, torch::kInt32, b, "dest");
  launch_segment_plan(pred.data_ptr<int64_t>(), b, nclasses, rowmap.numel(),
                      tseg.data_ptr<int>(), rowmap.data_ptr<int>(),
                      dest.data_ptr<int>(), cur_stream());
}

std::vector<torch::Tensor> segment_plan(torch::Tensor pred, int64_t nclasses) {
  TORCH_CHECK(pred.is_cuda() && pred.dim() == 1, "pred must be 1D on GPU");
  auto iopts = pred.options().dtype(torch::kInt32);
  auto tseg = torch::empty({nclasses + 1}, iopts);
  auto rowmap = torch::empty({segment_plan_rows(pred.size(0), nclasses)}, iopts);
  auto dest = torch::empty({pred.size(0)}, iopts);
  segment_plan_out(pred, nclasses, tseg, rowmap, dest);
  return {tseg, rowmap, dest};
}

// fp32 squared norms of bf16 rows. With `tseg`, rows at or past its last
// entry (the end of the last segment) are skipped.
void rownorm_bf16_out(torch::Tensor x, torch::Tensor out,
                      c10::optional<torch::Tensor> tseg) {
  TORCH_CHECK(x.dim() == 2, "x must be 2D");
  check_dev(x, torch::kBFloat16, x.numel(), "x");
  check_dev(out, torch::kFloat32, x.size(0), "out");
  const int* limit = nullptr;
  if (tseg.has_value()) {
    check_dev(tseg.value(), torch::kInt32, tseg.value().numel(), "tseg");
    TORCH_CHECK(tseg.value().numel() >= 1);
    limit = tseg.value().data_ptr<int>() + tseg.value().numel() - 1;
  }
  launch_rownorm_bf16(bf16_ptr(x), x.size(0), x.size(1), limit,
                      out.data_ptr<float>(), cur_stream());
}

void grouped_whiten_bf16(torch::Tensor ats, torch::Tensor rowmap,
                         torch::Tensor tseg, torch::Tensor wseg,
                         torch::Tensor keep, torch::Tensor wt,
                         torch::Tensor white) {
  TORCH_CHECK(ats.dim() == 2 && keep.dim() == 2 && wt.dim() == 3);
  const int64_t b = ats.size(0), dfull = ats.size(1);
  const int64_t c = keep.size(0), d = keep.size(1);
  const int64_t bp = segment_plan_rows(b, c);
  check_dev(ats, torch::kBFloat16, b * dfull, "ats");
  check_dev(rowmap, torch::kInt32, bp, "rowmap");
  check_dev(tseg, torch::kInt32, c + 1, "tseg");
  check_dev(wseg, torch::kInt32, c + 1, "wseg");
  check_dev(keep, torch::kInt32, c * d, "keep");
  // wt is [C, NP, KP]: out columns padded to 16, K padded to 32, zero-filled
  const int64_t np = wt.size(1), kp = wt.size(2);
  TORCH_CHECK(wt.size(0) == c && np % 16 == 0 && kp % 32 == 0 && np >= d &&
                  np < d + 16 && kp >= d && kp < d + 32,
              "wt must be [C, pad16(d), pad32(d)]");
  TORCH_CHECK(d >= 1 && kp <= grouped_whiten_max_features(),
              "grouped_whiten_bf16 supports up to ",
              grouped_whiten_max_features(), " features");
  check_dev(wt, torch::kBFloat16, c * np * kp, "wt");
  check_dev(white, torch::kBFloat16, bp * d, "white");
  launch_grouped_whiten_bf16(
      bf16_ptr(ats), b, dfull, rowmap.data_ptr<int>(), tseg.data_ptr<int>(),
      wseg.data_ptr<int>(), c, keep.data_ptr<int>(), bf16_ptr(wt), d, np, kp,
      bp, reinterpret_cast<short*>(white.data_ptr()), cur_stream());
}

void grouped_rowmin_plan(torch::Tensor ats, torch::Tensor trainS,
                         torch::Tensor tseg, torch::Tensor nseg,
                         torch::Tensor rowmap, torch::Tensor anorm,
                         torch::Tensor bnorm, torch::Tensor btable,
                         int64_t jb_max, torch::Tensor pval,
                         torch::Tensor pidx, torch::Tensor out_dsa,
                         torch::Tensor out_dist, torch::Tensor out_idx) {
  TORCH_CHECK(ats.dim() == 2 && trainS.dim() == 2 &&
              ats.size(1) == trainS.size(1), "feature dims differ");
  const int64_t b = ats.size(0), k = ats.size(1), n = trainS.size(0);
  const int64_t c = tseg.numel() - 1;
  const int64_t bp = segment_plan_rows(b, c);
  TORCH_CHECK(jb_max >= 1 && k % 8 == 0, "AT width must be a multiple of 8");
  check_dev(ats, torch::kBFloat16, b * k, "ats");
  check_dev(trainS, torch::kBFloat16, n * k, "trainS");
  check_dev(tseg, torch::kInt32, c + 1, "tseg");
  check_dev(nseg, torch::kInt32, c + 1, "nseg");
  check_dev(rowmap, torch::kInt32, bp, "rowmap");
  check_dev(anorm, torch::kFloat32, b, "anorm");
  check_dev(bnorm, torch::kFloat32, n, "bnorm");
  check_dev(btable, torch::kFloat32, n, "btable");
  check_dev(pval, torch::kFloat32, jb_max * bp, "pval");
  check_dev(pidx, torch::kInt32, jb_max * bp, "pidx");
  check_dev(out_dsa, torch::kFloat32, b, "out_dsa");
  check_dev(out_dist, torch::kFloat32, b, "out_dist");
  check_dev(out_idx, torch::kInt32, b, "out_idx");
  launch_grouped_rowmin_plan(
      bf16_ptr(ats), b, bf16_ptr(trainS), anorm.data_ptr<float>(),
      bnorm.data_ptr<float>(), tseg.data_ptr<int>(), nseg.data_ptr<int>(),
      rowmap.data_ptr<int>(), btable.data_ptr<float>(), c, bp, k, jb_max,
      pval.data_ptr<float>(), pidx.data_ptr<int>(),
      out_dsa.data_ptr<float>(), out_dist.data_ptr<float>(),
      out_idx.data_ptr<int>(), cur_stream());
}

void grouped_kde_plan(torch::Tensor white, torch::Tensor wtrain,
                      torch::Tensor tseg, torch::Tensor wseg,
                      torch::Tensor rowmap, torch::Tensor wanorm,
                      torch::Tensor wbnorm, torch::Tensor cls_fused,
                      torch::Tensor cls_const, int64_t jb_max,
                      torch::Tensor pkde, torch::Tensor out_lsa) {
  TORCH_CHECK(white.dim() == 2 && wtrain.dim() == 2 &&
              white.size(1) == wtrain.size(1), "feature dims differ");
  const int64_t bp = white.size(0), d = white.size(1), n = wtrain.size(0);
  const int64_t c = tseg.numel() - 1;
  const int64_t b = out_lsa.numel();
  TORCH_CHECK(jb_max >= 1 && bp == segment_plan_rows(b, c),
              "white does not match the plan");
  check_dev(white, torch::kBFloat16, bp * d, "white");
  check_dev(wtrain, torch::kBFloat16, n * d, "wtrain");
  check_dev(tseg, torch::kInt32, c + 1, "tseg");
  check_dev(wseg, torch::kInt32, c + 1, "wseg");
  check_dev(rowmap, torch::kInt32, bp, "rowmap");
  check_dev(wanorm, torch::kFloat32, bp, "wanorm");
  check_dev(wbnorm, torch::kFloat32, n, "wbnorm");
  check_dev(cls_fused, torch::kInt32, c, "cls_fused");
  check_dev(cls_const, torch::kFloat32, c, "cls_const");
  check_dev(pkde, torch::kFloat32, jb_max * bp * 2, "pkde");
  check_dev(out_lsa, torch::kFloat32, b, "out_lsa");
  launch_grouped_kde_plan(
      bf16_ptr(white), bf16_ptr(wtrain), wanorm.data_ptr<float>(),
      wbnorm.data_ptr<float>(), tseg.data_ptr<int>(), wseg.data_ptr<int>(),
      rowmap.data_ptr<int>(), b, cls_fused.data_ptr<int>(),
      cls_const.data_ptr<float>(), c, bp, d, jb_max,
      reinterpret_cast<float2*>(pkde.data_ptr<float>()),
      out_lsa.data_ptr<float>(), cur_stream());
}

// Grouped Gaussian scores through a segment plan made from the group ids:
// centre (segment.hip), quadratic forms + final scores (pairwise.hip). `out`
// must be pre-filled with +inf; rows the plan places nowhere keep it. With
// `logc` the score is the mixture NLL, without it the Mahalanobis form of the
// group's single component. `slots` is the largest component count of any
// group (a host constant of the tables, so nothing is read back here).
void grouped_gauss_plan(torch::Tensor x, torch::Tensor tseg,
                        torch::Tensor rowmap, torch::Tensor comp_off,
                        torch::Tensor means, torch::Tensor mats,
                        c10::optional<torch::Tensor> logc, int64_t slots,
                        torch::Tensor dc, torch::Tensor pquad,
                        torch::Tensor out) {
  TORCH_CHECK(x.dim() == 2 && means.dim() == 2 && mats.dim() == 3,
              "expected x [B, D], means [J, D], mats [J, D, D]");
  const int64_t b = x.size(0), d = x.size(1), j = means.size(0);
  const int64_t g = tseg.numel() - 1;
  const int64_t bp = segment_plan_rows(b, g);
  const int64_t jb = (d + kBN - 1) / kBN;
  TORCH_CHECK(b >= 1 && d >= 1 && j >= 1 && g >= 1, "empty operand");
  TORCH_CHECK(slots >= 1 && slots <= grouped_gauss_max_slots(),
              "at most ", grouped_gauss_max_slots(), " components per group");
  TORCH_CHECK(j * d < (1ll << 31) && slots * bp < (1ll << 31),
              "operand too large");
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  check_dev(x, bf16 ? torch::kBFloat16 : torch::kFloat32, b * d, "x");
  check_dev(tseg, torch::kInt32, g + 1, "tseg");
  check_dev(rowmap, torch::kInt32, bp, "rowmap");
  check_dev(comp_off, torch::kInt32, g + 1, "comp_off");
  check_dev(means, torch::kFloat32, j * d, "means");
  check_dev(mats, torch::kFloat32, j * d * d, "mats");
  check_dev(dc, torch::kFloat32, slots * bp * d, "dc");
  check_dev(pquad, torch::kFloat32, slots * jb * bp, "pquad");
  check_dev(out, torch::kFloat32, b, "out");
  const float* lc = nullptr;
  if (logc.has_value()) {
    check_dev(logc.value(), torch::kFloat32, j, "logc");
    lc = logc.value().data_ptr<float>();
  }
  if (d % 4 == 0) {
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % (bf16 ? 8 : 16) ==
                        0 &&
                    reinterpret_cast<uintptr_t>(means.data_ptr()) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(mats.data_ptr()) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(dc.data_ptr()) % 16 == 0,
                "operands must be 16-byte aligned");
  }
  launch_grouped_center(x.data_ptr(), bf16, b, d, rowmap.data_ptr<int>(),
                        tseg.data_ptr<int>(), comp_off.data_ptr<int>(), g, bp,
                        means.data_ptr<float>(), slots, dc.data_ptr<float>(),
                        cur_stream());
  launch_grouped_gauss_plan(dc.data_ptr<float>(), mats.data_ptr<float>(),
                            tseg.data_ptr<int>(), comp_off.data_ptr<int>(),
                            rowmap.data_ptr<int>(), b, lc, g, bp, d, slots,
                            pquad.data_ptr<float>(), out.data_ptr<float>(),
                            cur_stream());
}

torch::Tensor kde_logsumexp(torch::Tensor test, torch::Tensor train) {
  check_f32_2d(test, "test");
  check_f32_2d(train, "train");
  TORCH_CHECK(test.size(1) == train.size(1), "feature dims differ");
  TORCH_CHECK(train.size(0) > 0, "kde over empty train set");
  const int m = test.size(0), n = train.size(0), k = test.size(1);
  const int jb = (n + kBN - 1) / kBN;
  auto an = rownorm(test);
  auto bn = rownorm(train);
  auto pkde = torch::empty({jb, m, 2}, test.options());
  auto out = torch::empty({m}, test.options());
  launch_pairwise_kde(test.data_ptr<float>(), train.data_ptr<float>(),
                      an.data_ptr<float>(), bn.data_ptr<float>(), m, n, k,
                      reinterpret_cast<float2*>(pkde.data_ptr<float>()),
                      out.data_ptr<float>(), cur_stream());
  return out;
}

std::vector<torch::Tensor> profile(int mode, torch::Tensor acts,
                                   torch::Tensor lo, torch::Tensor hi,
                                   double thr, int64_t sections,
                                   int64_t nbits) {
  check_f32_2d(acts, "acts");
  const int rows = acts.size(0), K = acts.size(1);
  const int W = (nbits + 63) / 64;
  auto words = torch::empty({rows, W}, acts.options().dtype(torch::kInt64));
  auto scores = torch::empty({rows}, acts.options().dtype(torch::kInt64));
  const float* lop = lo.defined() && lo.numel() ? lo.data_ptr<float>() : nullptr;
  const float* hip = hi.defined() && hi.numel() ? hi.data_ptr<float>() : nullptr;
  launch_profile(mode, acts.data_ptr<float>(), nullptr, lop, hip,
                 static_cast<float>(thr), sections, rows, K, W,
                 reinterpret_cast<unsigned long long*>(words.data_ptr<int64_t>()),
                 reinterpret_cast<long long*>(scores.data_ptr<int64_t>()), cur_stream());
  return {words, scores};
}

torch::Tensor pack_bits(torch::Tensor boolmat) {
  TORCH_CHECK(boolmat.is_cuda() && boolmat.dtype() == torch::kBool &&
              boolmat.dim() == 2 && boolmat.is_contiguous());
  const int rows = boolmat.size(0), K = boolmat.size(1);
  const int W = (K + 63) / 64;
  auto words = torch::empty({rows, W},
                            boolmat.options().dtype(torch::kInt64));
  launch_profile(4 /*PROF_PACK*/, nullptr,
                 boolmat.data_ptr<bool>()
                     ? reinterpret_cast<const unsigned char*>(
                           boolmat.data_ptr<bool>())
                     : nullptr,
                 nullptr, nullptr, 0.f, 1, rows, K, W,
                 reinterpret_cast<unsigned long long*>(words.data_ptr<int64_t>()),
                 nullptr, cur_stream());
  return words;
}

torch::Tensor popcount_rows(torch::Tensor words) {
  TORCH_CHECK(words.is_cuda() && words.dtype() == torch::kInt64 &&
              words.dim() == 2 && words.is_contiguous());
  auto out = torch::empty({words.size(0)}, words.options());
  launch_popcount(
      reinterpret_cast<const unsigned long long*>(words.data_ptr<int64_t>()),
      words.size(0), words.size(1),
      reinterpret_cast<long long*>(out.data_ptr<int64_t>()), cur_stream());
  return out;
}

void tknc_layer(torch::Tensor layer, int64_t k, int64_t bit_offset,
                torch::Tensor words) {
  check_f32_2d(layer, "layer");
  TORCH_CHECK(k >= 1 && k <= 4, "tknc supports k in [1,4]");
  launch_tknc(layer.data_ptr<float>(), layer.size(0), layer.size(1), k,
              bit_offset, words.size(1),
              reinterpret_cast<unsigned long long*>(words.data_ptr<int64_t>()),
              cur_stream());
}

torch::Tensor bucketize(torch::Tensor values, torch::Tensor thresholds,
                        int64_t sections) {
  TORCH_CHECK(values.is_cuda() && values.dtype() == torch::kFloat64);
  TORCH_CHECK(thresholds.is_cuda() && thresholds.dtype() == torch::kFloat64);
  const int n = values.size(0);
  const int W = (sections + 63) / 64;
  auto words = torch::empty({n, W}, values.options().dtype(torch::kInt64));
  launch_bucketize(values.data_ptr<double>(), thresholds.data_ptr<double>(), n,
                   sections, W,
                   reinterpret_cast<unsigned long long*>(words.data_ptr<int64_t>()),
                   cur_stream());
  return words;
}

// Greedy CAM loop: the WHOLE loop runs in one persistent cooperative kernel
// (64 resident blocks + software grid barriers; profiles/r02_cam_ladder.md),
// whatever the mask width. The host reads the pick count and the picked
// prefix (rows that added coverage) once at the end.
torch::Tensor cam_greedy(torch::Tensor words, int64_t nbits) {
  TORCH_CHECK(words.is_cuda() && words.dtype() == torch::kInt64 &&
              words.dim() == 2 && words.is_contiguous());
  const int rows = words.size(0), W = words.size(1);
  auto opts = words.options();
  const int tail = nbits % 64;
  const unsigned long long tail_mask =
      tail ? ((1ull << tail) - 1) : ~0ull;
  auto used = torch::zeros({rows}, opts.dtype(torch::kUInt8));
  auto order_dev = torch::empty({rows}, opts);
  auto n_dev = torch::zeros({1}, opts.dtype(torch::kInt32));
  auto uncovered_dev = torch::empty({W}, opts);  // the kernel initialises it
  auto part_val = torch::empty({64}, opts);
  auto part_idx = torch::empty({64}, opts.dtype(torch::kInt32));
  auto aux = torch::zeros({2}, opts.dtype(torch::kInt32));  // barrier, win
  launch_cam_greedy_coop(
      reinterpret_cast<const unsigned long long*>(words.data_ptr<int64_t>()),
      rows, W, tail_mask, used.data_ptr<uint8_t>(),
      reinterpret_cast<unsigned long long*>(
          uncovered_dev.data_ptr<int64_t>()),
      reinterpret_cast<long long*>(part_val.data_ptr<int64_t>()),
      part_idx.data_ptr<int>(),
      reinterpret_cast<long long*>(order_dev.data_ptr<int64_t>()),
      n_dev.data_ptr<int>(), aux.data_ptr<int>(), aux.data_ptr<int>() + 1,
      cur_stream());
  const int n = n_dev.cpu().item<int>();
  return order_dev.narrow(0, 0, n).cpu();
}

// Batched CAM (cam_many.hip): the greedy loops of 1..CAM_MANY_MAX_PROBLEMS
// problems in one persistent launch, one team of blocks per problem. The
// profile matrices are read where they lie. One device-to-host copy brings
// every pick count and status word; the picked prefixes stay on the device
// and are returned as views of one buffer. A problem whose bounded wait ran
// out raises, no partial order is returned.
// Measurement switch (scripts/perf_cam_many.py): no pick publishes a list, so
// every sweep recounts against the whole mask. Orders do not change.
bool g_cam_many_force_full = false;
void cam_many_force_full(bool on) { g_cam_many_force_full = on; }

std::vector<torch::Tensor> cam_greedy_many(std::vector<torch::Tensor> words,
                                           std::vector<int64_t> nbits) {
  const int P = (int)words.size();
  TORCH_CHECK(P >= 1 && P <= CAM_MANY_MAX_PROBLEMS && (int)nbits.size() == P,
              "cam_greedy_many takes 1..", CAM_MANY_MAX_PROBLEMS,
              " problems per call");
  std::vector<int64_t> rows(P), Ws(P);
  for (int p = 0; p < P; ++p) {
    const auto& w = words[p];
    TORCH_CHECK(w.is_cuda() && w.dtype() == torch::kInt64 && w.dim() == 2 &&
                    w.is_contiguous() && w.device() == words[0].device(),
                "cam_greedy_many: words[", p,
                "] must be a contiguous int64 [N, W] tensor on one device");
    rows[p] = w.size(0);
    Ws[p] = w.size(1);
    // the barrier counter (2 * rows * team) and the gains (W * 64) are ints
    TORCH_CHECK(rows[p] >= 1 && rows[p] < (1 << 23) && Ws[p] >= 1 &&
                    Ws[p] < (1 << 24) && Ws[p] == (nbits[p] + 63) / 64,
                "cam_greedy_many: problem ", p, " is outside the envelope");
  }
  const int grid = cam_many_grid();
  TORCH_CHECK(grid >= P, "cam_greedy_many: ", P, " problems need ", P,
              " CUs, the device reports ", grid);
  const std::vector<int> team = cam_many_teams(rows, Ws, grid);

  int64_t n_rows = 0, n_words = 0, n_list = 0, n_team = 0;
  std::vector<int> list_cap(P);
  for (int p = 0; p < P; ++p) {
    list_cap[p] = g_cam_many_force_full
                      ? 0
                      : (int)std::min<int64_t>(Ws[p] / CAM_MANY_INCR_DIV,
                                               CAM_MANY_LIST_CAP);
    n_rows += rows[p];
    n_words += Ws[p];
    n_list += 2 * list_cap[p];
    n_team += team[p];
  }
  auto o64 = words[0].options();
  auto o32 = o64.dtype(torch::kInt32);
  // [counts P | status P | orders]; only the head is zeroed and read back
  auto res = torch::empty({2 * P + n_rows}, o64);
  res.narrow(0, 0, 2 * P).zero_();
  auto ws64 = torch::empty({n_words + n_list}, o64);        // masks, lists
  auto ws32 = torch::empty({n_rows + 2 * n_team}, o32);     // gains, maxima
  auto sync = torch::zeros({(int64_t)P * CAM_MANY_SYNC_WORDS}, o32);

  std::vector<CamManyDesc> table(P);
  auto* res_p = reinterpret_cast<long long*>(res.data_ptr<int64_t>());
  auto* w64 = reinterpret_cast<unsigned long long*>(ws64.data_ptr<int64_t>());
  int* w32 = ws32.data_ptr<int>();
  int64_t at_row = 0, at_word = 0, at_list = 0, at_team = 0;
  for (int p = 0; p < P; ++p) {
    CamManyDesc& d = table[p];
    const int tail = (int)(nbits[p] % 64);
    d.words = reinterpret_cast<const unsigned long long*>(
        words[p].data_ptr<int64_t>());
    d.uncovered = w64 + at_word;
    d.list = w64 + n_words + at_list;
    d.gain = w32 + at_row;
    d.part_val = w32 + n_rows + at_team;
    d.part_idx = w32 + n_rows + n_team + at_team;
    d.order = res_p + 2 * P + at_row;
    d.count = res_p + p;
    d.status = res_p + P + p;
    d.sync = sync.data_ptr<int>() + (int64_t)p * CAM_MANY_SYNC_WORDS;
    d.tail_mask = tail ? ((1ull << tail) - 1) : ~0ull;
    d.rows = (int)rows[p];
    d.W = (int)Ws[p];
    d.first_block = (int)at_team;
    d.team = team[p];
    d.list_cap = list_cap[p];
    d.wide = Ws[p] >= CAM_MANY_WIDE_WORDS;
    at_row += rows[p];
    at_word += Ws[p];
    at_list += 2 * list_cap[p];
    at_team += team[p];
  }
  TORCH_CHECK(at_team <= grid, "cam_greedy_many: team plan exceeds the grid");
  auto table_dev =
      torch::from_blob(table.data(), {(int64_t)(P * sizeof(CamManyDesc))},
                       torch::dtype(torch::kUInt8))
          .to(words[0].device());
  launch_cam_many(reinterpret_cast<const CamManyDesc*>(
                      table_dev.data_ptr<uint8_t>()),
                  P, grid, cur_stream());
  const auto head = res.narrow(0, 0, 2 * P).cpu();  // waits for the launch
  const int64_t* h = head.data_ptr<int64_t>();
  for (int p = 0; p < P; ++p)
    TORCH_CHECK(h[P + p] == 0, "cam_greedy_many: problem ", p, " (", rows[p],
                " x ", Ws[p], " words, team of ", team[p],
                " blocks) ran into the bound of a team-barrier wait; no "
                "order is returned");
  std::vector<torch::Tensor> out(P);
  at_row = 0;
  for (int p = 0; p < P; ++p) {
    out[p] = res.narrow(0, 2 * P + at_row, h[p]);
    at_row += rows[p];
  }
  return out;
}

std::vector<int64_t> cam_many_plan(std::vector<int64_t> rows,
                                   std::vector<int64_t> W, int64_t grid) {
  TORCH_CHECK(rows.size() == W.size() && (int64_t)rows.size() <= grid);
  const std::vector<int> team = cam_many_teams(rows, W, (int)grid);
  return std::vector<int64_t>(team.begin(), team.end());
}

int64_t cam_many_max_problems() { return CAM_MANY_MAX_PROBLEMS; }
int64_t cam_many_wide_words() { return CAM_MANY_WIDE_WORDS; }
int64_t cam_many_incr_div() { return CAM_MANY_INCR_DIV; }
int64_t cam_many_list_cap() { return CAM_MANY_LIST_CAP; }
int64_t cam_many_team_cap() { return CAM_MANY_TEAM_CAP; }

// All-pairs Levenshtein distance matrix (CPU, threaded) for the text
// corruptor's autocorrect dictionary (the reference uses the
// polyleven pip package on a thread pool, text_corruptor.py:282-309).
torch::Tensor levenshtein_matrix(std::vector<std::string> words) {
  const int64_t n = (int64_t)words.size();
  auto out = torch::zeros({n, n}, torch::dtype(torch::kUInt8));
  auto acc = out.accessor<uint8_t, 2>();
  at::parallel_for(0, n, 1, [&](int64_t begin, int64_t end) {
    std::vector<int> dp0(64), dp1(64);
    for (int64_t i = begin; i < end; ++i) {
      const std::string& a = words[i];
      const int la = (int)a.size();
      for (int64_t j = i + 1; j < n; ++j) {
        const std::string& b = words[j];
        const int lb = (int)b.size();
        if (lb + 1 > (int)dp0.size()) {
          dp0.resize(lb + 1);
          dp1.resize(lb + 1);
        }
        for (int c = 0; c <= lb; ++c) dp0[c] = c;
        for (int r = 1; r <= la; ++r) {
          dp1[0] = r;
          const char ca = a[r - 1];
          for (int c = 1; c <= lb; ++c) {
            const int sub = dp0[c - 1] + (ca != b[c - 1] ? 1 : 0);
            const int del = dp0[c] + 1;
            const int ins = dp1[c - 1] + 1;
            dp1[c] = std::min(sub, std::min(del, ins));
          }
          std::swap(dp0, dp1);
        }
        const int d = std::min(dp0[lb], 255);
        acc[i][j] = (uint8_t)d;
        acc[j][i] = (uint8_t)d;
      }
    }
  });
  return out;
}

std::vector<torch::Tensor> softmax_scores(torch::Tensor probs) {
  check_f32_2d(probs, "probs");
  const int n = probs.size(0), c = probs.size(1);
  auto neg_max = torch::empty({n}, probs.options());
  auto neg_pcs = torch::empty({n}, probs.options());
  auto entropy = torch::empty({n}, probs.options());
  auto gini = torch::empty({n}, probs.options());
  launch_softmax_scores(probs.data_ptr<float>(), n, c,
                        neg_max.data_ptr<float>(), neg_pcs.data_ptr<float>(),
                        entropy.data_ptr<float>(), gini.data_ptr<float>(),
                        cur_stream());
  return {neg_max, neg_pcs, entropy, gini};
}

// ---- fused ResNet-20 inference (bf16 NHWC) ----

const short* bf16_ptr(const torch::Tensor& t) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kBFloat16 && t.is_contiguous());
  return reinterpret_cast<const short*>(t.data_ptr());
}

torch::Tensor mfma_probe(torch::Tensor a, torch::Tensor b) {
  auto d = torch::empty({16, 16}, a.options().dtype(torch::kFloat32));
  launch_mfma_probe(bf16_ptr(a), bf16_ptr(b),
                    d.data_ptr<float>(), cur_stream());
  return d;
}

torch::Tensor resnet_block(int64_t variant, torch::Tensor x, torch::Tensor w1,
                           torch::Tensor b1, torch::Tensor w2, torch::Tensor b2) {
  const int batch = x.size(0);
  auto out = torch::empty_like(x);
  launch_resblock(variant, batch, bf16_ptr(x),
                  const_cast<short*>(bf16_ptr(out)), bf16_ptr(w1),
                  b1.data_ptr<float>(), bf16_ptr(w2), b2.data_ptr<float>(),
                  cur_stream());
  return out;
}

torch::Tensor resnet_down(int64_t variant, torch::Tensor x, torch::Tensor w1,
                          torch::Tensor b1, torch::Tensor w2, torch::Tensor b2,
                          torch::Tensor wsc, torch::Tensor bsc) {
  const int batch = x.size(0);
  const int64_t out_elems = x.size(1) / 2;  // H*W*C -> (H/2)(W/2)(2C)
  auto out = torch::empty({batch, out_elems}, x.options());
  launch_downblock(variant, batch, bf16_ptr(x),
                   const_cast<short*>(bf16_ptr(out)), bf16_ptr(w1),
                   b1.data_ptr<float>(), bf16_ptr(w2), b2.data_ptr<float>(),
                   bf16_ptr(wsc), bsc.data_ptr<float>(), cur_stream());
  return out;
}

torch::Tensor resnet_stem(torch::Tensor x, torch::Tensor w, torch::Tensor b) {
  const int batch = x.size(0);
  const int64_t out_elems = 32 * 32 * 16;
  auto out = torch::empty({batch, out_elems}, x.options());
  launch_stem(batch, bf16_ptr(x), const_cast<short*>(bf16_ptr(out)),
              bf16_ptr(w), b.data_ptr<float>(), cur_stream());
  return out;
}

// ---- stage-resident forward: three kernels, planes stay in LDS ----

// Collects a stage's parameter pointers in forward order and checks each
// tensor's size against the shapes the kernel is compiled for.
struct StageParams {
  const std::vector<torch::Tensor>& t;
  size_t next = 0;
  std::vector<const void*> ptrs;

  explicit StageParams(const std::vector<torch::Tensor>& params) : t(params) {}

  const torch::Tensor& take() {
    TORCH_CHECK(next < t.size(), "too few stage parameters");
    return t[next++];
  }
  // packed conv weight [cout/16][ceil(k/32)][64][8] bf16, then fp32 bias
  void conv(int64_t k, int64_t cout) {
    const torch::Tensor& w = take();
    TORCH_CHECK(w.numel() == (cout / 16) * ((k + 31) / 32) * 512,
                "packed conv weight has the wrong size");
    ptrs.push_back(bf16_ptr(w));
    f32(cout);
  }
  void f32(int64_t n) {
    const torch::Tensor& b = take();
    TORCH_CHECK(b.is_cuda() && b.dtype() == torch::kFloat32 &&
                    b.is_contiguous() && b.numel() == n,
                "fp32 stage parameter has the wrong type or size");
    ptrs.push_back(b.data_ptr<float>());
  }
  void res(int64_t c) {
    conv(9 * c, c);
    conv(9 * c, c);
  }
  void down(int64_t c) {
    conv(9 * c, 2 * c);
    conv(18 * c, 2 * c);
    conv(c, 2 * c);
  }
  const void* const* done() {
    TORCH_CHECK(next == t.size(), "too many stage parameters");
    return ptrs.data();
  }
};

void check_plane(const torch::Tensor& x, int64_t elems) {
  TORCH_CHECK(x.dim() == 2 && x.size(1) == elems, "x must be [B, ", elems, "]");
}

// x: fp32 [B, 32, 32, 3] contiguous. params: stem w, b; 3 x (w1, b1, w2, b2);
// down w1, b1, w2, b2, wsc, bsc. Returns the stage-1 plane bf16 [B, 16*16*32].
torch::Tensor resnet_stage1(torch::Tensor x,
                            std::vector<torch::Tensor> params) {
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kFloat32 &&
                  x.is_contiguous() && x.dim() == 4 && x.size(1) == 32 &&
                  x.size(2) == 32 && x.size(3) == 3,
              "x must be a contiguous fp32 [B, 32, 32, 3] GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "x must be 16-byte aligned");
  StageParams p(params);
  p.conv(9 * 8, 16);
  for (int i = 0; i < 3; ++i) p.res(16);
  p.down(16);
  const void* const* ptrs = p.done();
  const int batch = x.size(0);
  auto out = torch::empty({batch, 16 * 16 * 32},
                          x.options().dtype(torch::kBFloat16));
  if (batch > 0)
    launch_stage1(batch, x.data_ptr<float>(),
                  const_cast<short*>(bf16_ptr(out)), ptrs, cur_stream());
  return out;
}

// x: bf16 [B, 16*16*32]. params: 2 x (w1, b1, w2, b2); down (6).
// Returns the stage-2 plane bf16 [B, 8*8*64].
torch::Tensor resnet_stage2(torch::Tensor x,
                            std::vector<torch::Tensor> params) {
  check_plane(x, 16 * 16 * 32);
  StageParams p(params);
  for (int i = 0; i < 2; ++i) p.res(32);
  p.down(32);
  const void* const* ptrs = p.done();
  const int batch = x.size(0);
  auto out = torch::empty({batch, 8 * 8 * 64}, x.options());
  if (batch > 0)
    launch_stage2(batch, bf16_ptr(x), const_cast<short*>(bf16_ptr(out)), ptrs,
                  cur_stream());
  return out;
}

// x: bf16 [B, 8*8*64]. params: 2 x (w1, b1, w2, b2); fc w [10, 64], b [10].
// Returns (stage-3 ATs bf16 [B, 4096], logits fp32 [B, 10]).
std::vector<torch::Tensor> resnet_stage3(torch::Tensor x,
                                         std::vector<torch::Tensor> params) {
  check_plane(x, 8 * 8 * 64);
  StageParams p(params);
  for (int i = 0; i < 2; ++i) p.res(64);
  p.f32(10 * 64);
  p.f32(10);
  const void* const* ptrs = p.done();
  const int batch = x.size(0);
  auto ats = torch::empty_like(x);
  auto logits = torch::empty({batch, 10}, x.options().dtype(torch::kFloat32));
  if (batch > 0)
    launch_stage3(batch, bf16_ptr(x), const_cast<short*>(bf16_ptr(ats)),
                  logits.data_ptr<float>(), ptrs, cur_stream());
  return {ats, logits};
}

// ---- fused MC-dropout head (variation-ratio votes) ----

// thresh = floor(p * 2^32) and scale = float32(1 / (1 - p)) are computed once
// by the Python wrapper so the CPU oracle and the kernel share the exact bits.
// Argument checks shared by mc_dropout_votes and mc_dropout_stats.
static void mc_dropout_check(const torch::Tensor& feats,
                             const torch::Tensor& weight,
                             const torch::Tensor& bias, int64_t thresh,
                             int64_t num_samples, int64_t row_offset) {
  check_f32_2d(feats, "feats");
  check_f32_2d(weight, "weight");
  TORCH_CHECK(bias.is_cuda() && bias.dtype() == torch::kFloat32 &&
                  bias.dim() == 1 && bias.is_contiguous(),
              "bias must be a contiguous 1D fp32 GPU tensor");
  const int64_t n = feats.size(0), d = feats.size(1), c = weight.size(0);
  TORCH_CHECK(weight.size(1) == d, "weight must be [C, D]");
  TORCH_CHECK(bias.size(0) == c, "bias must be [C]");
  TORCH_CHECK(c >= 1 && c <= mc_dropout_max_classes() && d >= 1 &&
                  d <= mc_dropout_max_features(),
              "mc_dropout_votes envelope is C <= ", mc_dropout_max_classes(),
              ", D <= ", mc_dropout_max_features());
  TORCH_CHECK(num_samples >= 1 && num_samples <= 65535, "bad num_samples");
  TORCH_CHECK(thresh >= 0 && thresh <= 0xFFFFFFFFll, "bad threshold");
  TORCH_CHECK(n <= 0x7FFFFFFFll && row_offset >= 0 &&
                  row_offset + n <= 0x100000000ll,
              "rows must satisfy row_offset + N <= 2^32");
}

torch::Tensor mc_dropout_votes(torch::Tensor feats, torch::Tensor weight,
                               torch::Tensor bias, int64_t thresh,
                               double scale, int64_t num_samples,
                               int64_t seed_lo, int64_t seed_hi,
                               int64_t row_offset) {
  mc_dropout_check(feats, weight, bias, thresh, num_samples, row_offset);
  const int64_t n = feats.size(0), d = feats.size(1), c = weight.size(0);
  auto votes = torch::empty({n, c}, feats.options().dtype(torch::kInt32));
  if (n == 0) return votes;
  launch_mc_dropout_votes(
      feats.data_ptr<float>(), weight.data_ptr<float>(),
      bias.data_ptr<float>(), (int)n, (int)d, (int)c, (int)num_samples,
      (uint32_t)thresh, (float)scale, (uint32_t)seed_lo, (uint32_t)seed_hi,
      (uint32_t)row_offset, votes.data_ptr<int>(), cur_stream());
  return votes;
}

// votes as above plus the mean softmax [N, C] and the mean per-sample
// entropy [N] of the same S masked heads, from one launch.
std::vector<torch::Tensor> mc_dropout_stats(
    torch::Tensor feats, torch::Tensor weight, torch::Tensor bias,
    int64_t thresh, double scale, int64_t num_samples, int64_t seed_lo,
    int64_t seed_hi, int64_t row_offset) {
  mc_dropout_check(feats, weight, bias, thresh, num_samples, row_offset);
  const int64_t n = feats.size(0), d = feats.size(1), c = weight.size(0);
  auto votes = torch::empty({n, c}, feats.options().dtype(torch::kInt32));
  auto mean_probs = torch::empty({n, c}, feats.options());
  auto mean_entropy = torch::empty({n}, feats.options());
  if (n == 0) return {votes, mean_probs, mean_entropy};
  launch_mc_dropout_stats(
      feats.data_ptr<float>(), weight.data_ptr<float>(),
      bias.data_ptr<float>(), (int)n, (int)d, (int)c, (int)num_samples,
      (uint32_t)thresh, (float)scale, (uint32_t)seed_lo, (uint32_t)seed_hi,
      (uint32_t)row_offset, votes.data_ptr<int>(),
      mean_probs.data_ptr<float>(), mean_entropy.data_ptr<float>(),
      cur_stream());
  return {votes, mean_probs, mean_entropy};
}

// ---- fused MC-dropout transformer tail (four dropout sites) ----

// {E, max T, max F, max H, max C} of the kernel envelope.
std::vector<int64_t> mc_transformer_envelope() {
  int lim[5];
  mc_transformer_limits(lim);
  return {lim[0], lim[1], lim[2], lim[3], lim[4]};
}

// params: ln1_w, ln1_b, w1 [F,E], b1, w2 [E,F], b2, ln2_w, ln2_b, w3 [H,E],
// b3, w4 [C,H], b4. Returns {votes} or {votes, mean_probs, mean_entropy}.
std::vector<torch::Tensor> mc_transformer(
    torch::Tensor x, torch::Tensor attn, std::vector<torch::Tensor> params,
    double eps, std::vector<int64_t> thresh, std::vector<double> scale,
    int64_t num_samples, int64_t seed_lo, int64_t seed_hi, int64_t row_offset,
    bool with_stats) {
  int lim[5];
  mc_transformer_limits(lim);
  TORCH_CHECK(x.is_cuda() && x.dtype() == torch::kFloat32 && x.dim() == 3 &&
                  x.is_contiguous(),
              "x must be a contiguous [N, T, E] fp32 GPU tensor");
  TORCH_CHECK(attn.is_cuda() && attn.dtype() == torch::kFloat32 &&
                  attn.is_contiguous() && attn.sizes() == x.sizes(),
              "attn must be a contiguous fp32 GPU tensor shaped like x");
  TORCH_CHECK(params.size() == 12 && thresh.size() == 4 && scale.size() == 4,
              "expected 12 parameter tensors and 4 rates");
  const int64_t n = x.size(0), t = x.size(1), e = x.size(2);
  for (const auto& p : params)
    TORCH_CHECK(p.is_cuda() && p.dtype() == torch::kFloat32 &&
                    p.is_contiguous() && p.dim() >= 1 && p.dim() <= 2,
                "parameters must be contiguous fp32 GPU tensors");
  TORCH_CHECK(params[2].dim() == 2 && params[8].dim() == 2 &&
                  params[10].dim() == 2,
              "w1, w3 and w4 must be 2-D");
  const int64_t f = params[2].size(0), h = params[8].size(0),
                c = params[10].size(0);
  TORCH_CHECK(e == lim[0] && t >= 1 && t <= lim[1] && f >= 1 && f <= lim[2] &&
                  h >= 1 && h <= lim[3] && c >= 1 && c <= lim[4],
              "mc_transformer envelope is E == ", lim[0], ", T <= ", lim[1],
              ", F <= ", lim[2], ", H <= ", lim[3], ", C <= ", lim[4]);
  const int64_t want[12][2] = {{e, 0}, {e, 0}, {f, e}, {f, 0}, {e, f}, {e, 0},
                               {e, 0}, {e, 0}, {h, e}, {h, 0}, {c, h}, {c, 0}};
  for (int i = 0; i < 12; ++i) {
    const bool two = want[i][1] != 0;
    TORCH_CHECK(params[i].dim() == (two ? 2 : 1) &&
                    params[i].size(0) == want[i][0] &&
                    (!two || params[i].size(1) == want[i][1]),
                "parameter ", i, " has the wrong shape");
  }
  TORCH_CHECK(num_samples >= 1 && num_samples <= 65535, "bad num_samples");
  uint32_t th[4];
  float sc[4];
  for (int i = 0; i < 4; ++i) {
    TORCH_CHECK(thresh[i] >= 0 && thresh[i] <= 0xFFFFFFFFll, "bad threshold");
    th[i] = (uint32_t)thresh[i];
    sc[i] = (float)scale[i];
  }
  TORCH_CHECK(n <= 0x7FFFFFFFll && row_offset >= 0 &&
                  row_offset + n <= 0x100000000ll,
              "rows must satisfy row_offset + N <= 2^32");
  auto votes = torch::empty({n, c}, x.options().dtype(torch::kInt32));
  torch::Tensor mean_probs, mean_entropy;
  if (with_stats) {
    mean_probs = torch::empty({n, c}, x.options());
    mean_entropy = torch::empty({n}, x.options());
  }
  if (n > 0) {
    const float* ptrs[12];
    for (int i = 0; i < 12; ++i) ptrs[i] = params[i].data_ptr<float>();
    launch_mc_transformer(
        x.data_ptr<float>(), attn.data_ptr<float>(), ptrs, (float)eps, th, sc,
        (int)n, (int)t, (int)f, (int)h, (int)c, (int)num_samples,
        (uint32_t)seed_lo, (uint32_t)seed_hi, (uint32_t)row_offset,
        votes.data_ptr<int>(),
        with_stats ? mean_probs.data_ptr<float>() : nullptr,
        with_stats ? mean_entropy.data_ptr<float>() : nullptr, with_stats,
        cur_stream());
  }
  if (with_stats) return {votes, mean_probs, mean_entropy};
  return {votes};
}

// ---- fused coverage suite (coverage_suite.hip) ----

// Every NAC / SNAC / NBC / KMNC / TKNC profile of `layers` ([N, K_l] fp32
// each, not concatenated) in two launches. Returns one words tensor per
// profile in the order NAC, SNAC, NBC, KMNC, TKNC, then scores [profiles, N].
// The Python wrapper checks the envelope and raises ValueError; the checks
// here guard the kernels' indexing.
std::vector<torch::Tensor> coverage_suite(
    std::vector<torch::Tensor> layers, std::vector<double> nac_thresholds,
    torch::Tensor snac_hi, torch::Tensor nbc_lo, torch::Tensor nbc_hi,
    torch::Tensor kmnc_lo, torch::Tensor kmnc_hi,
    std::vector<int64_t> kmnc_sections, std::vector<int64_t> tknc_ks) {
  const int64_t L = layers.size();
  TORCH_CHECK(L >= 1 && L <= SUITE_MAX_LAYERS, "coverage_suite takes 1..",
              SUITE_MAX_LAYERS, " layers");
  const int64_t n = layers[0].size(0);
  SuiteArgs a = {};
  SuiteTopkArgs tk = {};
  int64_t K = 0;
  for (int64_t l = 0; l < SUITE_MAX_LAYERS; ++l) {
    a.off[l] = tk.off[l] = INT_MAX;
    if (l >= L) continue;
    check_f32_2d(layers[l], "layer");
    TORCH_CHECK(layers[l].size(0) == n, "layers must share N");
    a.layer[l] = tk.layer[l] = layers[l].data_ptr<float>();
    a.off[l] = tk.off[l] = (int)K;
    a.width[l] = tk.width[l] = (int)layers[l].size(1);
    K += layers[l].size(1);
    TORCH_CHECK(K * SUITE_MAX_SECTIONS < INT_MAX, "too many neurons");
  }
  TORCH_CHECK(n < INT_MAX, "too many rows");
  TORCH_CHECK((K + coverage_suite_chunk() - 1) / coverage_suite_chunk() <= 65535,
              "too many neurons");
  const int64_t n_nac = nac_thresholds.size(), n_kmnc = kmnc_sections.size();
  const int64_t n_tknc = tknc_ks.size();
  const int64_t n_snac = snac_hi.numel() ? snac_hi.size(0) : 0;
  const int64_t n_nbc = nbc_lo.numel() ? nbc_lo.size(0) : 0;
  TORCH_CHECK(n_nac <= SUITE_MAX_FAMILY && n_snac <= SUITE_MAX_FAMILY &&
                  n_nbc <= SUITE_MAX_FAMILY && n_kmnc <= SUITE_MAX_FAMILY &&
                  n_tknc <= SUITE_MAX_FAMILY,
              "at most ", SUITE_MAX_FAMILY, " profiles per family");
  if (n_snac) check_dev(snac_hi, torch::kFloat32, n_snac * K, "upper_bounds");
  if (n_nbc) {
    check_dev(nbc_lo, torch::kFloat32, n_nbc * K, "nbc_lower");
    check_dev(nbc_hi, torch::kFloat32, n_nbc * K, "nbc_upper");
  }
  if (n_kmnc) {
    check_dev(kmnc_lo, torch::kFloat32, K, "kmnc_mins");
    check_dev(kmnc_hi, torch::kFloat32, K, "kmnc_maxs");
  }
  for (int64_t s : kmnc_sections)
    TORCH_CHECK(s >= 1 && s <= SUITE_MAX_SECTIONS, "kmnc sections in 1..",
                SUITE_MAX_SECTIONS);
  for (int64_t k : tknc_ks)
    TORCH_CHECK(k >= 1 && k <= SUITE_MAX_TOPK, "tknc k in 1..", SUITE_MAX_TOPK);

  // words per row of every profile, in output order
  const int64_t w_flat = (K + 63) / 64;
  std::vector<int64_t> widths;
  for (int64_t i = 0; i < n_nac + n_snac; ++i) widths.push_back(w_flat);
  for (int64_t i = 0; i < n_nbc; ++i) widths.push_back((2 * K + 63) / 64);
  for (int64_t s : kmnc_sections) widths.push_back((K * s + 63) / 64);
  const int64_t n_thr = widths.size(), n_prof = n_thr + n_tknc;
  int64_t thr_words = 0;
  for (int64_t w : widths) thr_words += n * w;

  // the threshold kernel writes every word it owns; scores and the TKNC
  // words are accumulated into, so they start at zero (one fill for both)
  auto iopts = layers[0].options().dtype(torch::kInt64);
  auto thr_buf = torch::empty({thr_words}, iopts);
  auto zero_buf = torch::zeros({n_prof * n + n_tknc * n * w_flat}, iopts);
  auto scores = zero_buf.narrow(0, 0, n_prof * n).view({n_prof, n});
  std::vector<torch::Tensor> out;
  int64_t at = 0;
  for (int64_t i = 0; i < n_thr; ++i) {
    out.push_back(thr_buf.narrow(0, at, n * widths[i]).view({n, widths[i]}));
    at += n * widths[i];
  }
  for (int64_t t = 0; t < n_tknc; ++t)
    out.push_back(zero_buf.narrow(0, n_prof * n + t * n * w_flat, n * w_flat)
                      .view({n, w_flat}));
  out.push_back(scores);
  if (n == 0 || K == 0) return out;

  auto wptr = [](torch::Tensor& t) {
    return reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>());
  };
  if (n_thr > 0) {
    a.rows = (int)n;
    a.K = (int)K;
    a.n_nac = (int)n_nac;
    a.n_snac = (int)n_snac;
    a.n_nbc = (int)n_nbc;
    a.n_kmnc = (int)n_kmnc;
    int64_t p = 0;
    for (int64_t i = 0; i < n_nac; ++i) {
      a.nac_thr[i] = static_cast<float>(nac_thresholds[i]);
      a.words[i] = wptr(out[p++]);
    }
    for (int64_t i = 0; i < n_snac; ++i)
      a.words[SUITE_MAX_FAMILY + i] = wptr(out[p++]);
    for (int64_t i = 0; i < n_nbc; ++i)
      a.words[2 * SUITE_MAX_FAMILY + i] = wptr(out[p++]);
    for (int64_t i = 0; i < n_kmnc; ++i) {
      a.kmnc_sec[i] = (int)kmnc_sections[i];
      a.words[3 * SUITE_MAX_FAMILY + i] = wptr(out[p++]);
    }
    a.snac_hi = n_snac ? snac_hi.data_ptr<float>() : nullptr;
    a.nbc_lo = n_nbc ? nbc_lo.data_ptr<float>() : nullptr;
    a.nbc_hi = n_nbc ? nbc_hi.data_ptr<float>() : nullptr;
    a.kmnc_lo = n_kmnc ? kmnc_lo.data_ptr<float>() : nullptr;
    a.kmnc_hi = n_kmnc ? kmnc_hi.data_ptr<float>() : nullptr;
    a.scores = reinterpret_cast<long long*>(scores.data_ptr<int64_t>());
    launch_coverage_suite_threshold(a, cur_stream());
  }
  if (n_tknc > 0) {
    tk.rows = (int)n;
    tk.L = (int)L;
    tk.W = (int)w_flat;
    tk.n = (int)n_tknc;
    for (int64_t t = 0; t < n_tknc; ++t) {
      tk.k[t] = (int)tknc_ks[t];
      tk.words[t] = wptr(out[n_thr + t]);
      tk.scores[t] = reinterpret_cast<long long*>(scores.data_ptr<int64_t>()) +
                     (n_thr + t) * n;
    }
    launch_coverage_suite_topk(tk, cur_stream());
  }
  return out;
}

int64_t coverage_suite_chunk_py() { return coverage_suite_chunk(); }

// ---- batched k-means (kmeans_many.hip, silhouette epilogue of pairwise.hip).
// Shapes and the envelope are validated by ops/hip_ops.py; the checks here
// only keep a wrong call from reaching a kernel.

void check_i32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dtype() == torch::kInt32 && t.is_contiguous(),
              name, " must be a contiguous int32 GPU tensor");
}

void check_kmeans_many(const torch::Tensor& x, const torch::Tensor& seg,
                       int64_t c) {
  check_f32_2d(x, "x");
  check_i32(seg, "seg");
  const int64_t p = seg.numel() - 1;
  TORCH_CHECK(p >= 1 && p <= KMEANS_MANY_MAX_PROBLEMS, "1..",
              KMEANS_MANY_MAX_PROBLEMS, " problems");
  TORCH_CHECK(c >= 1 && c <= KMEANS_MANY_MAX_CENTERS, "1..",
              KMEANS_MANY_MAX_CENTERS, " centres");
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) < (1 << 24) && x.size(1) >= 1,
              "x must have 1 .. 2^24 - 1 rows");
}

std::vector<torch::Tensor> lloyd_assign_many(
    torch::Tensor x, torch::Tensor centers, torch::Tensor seg,
    c10::optional<torch::Tensor> xnorm) {
  check_f32_2d(centers, "centers");
  check_kmeans_many(x, seg, centers.size(0));
  TORCH_CHECK(x.size(1) == centers.size(1), "feature dims differ");
  const int n = x.size(0), c = centers.size(0), d = x.size(1);
  const int p = seg.numel() - 1;
  auto xn = xnorm.has_value() ? xnorm.value() : rownorm(x);
  TORCH_CHECK(xn.is_cuda() && xn.dtype() == torch::kFloat32 &&
              xn.is_contiguous() && xn.numel() == n, "xnorm must be fp32 [N]");
  auto cn = rownorm(centers);
  auto d2 = torch::empty({n, c}, x.options());
  auto labels = torch::empty({p, n}, x.options().dtype(torch::kInt32));
  auto mind = torch::empty({p, n}, x.options());
  launch_pairwise_full(x.data_ptr<float>(), centers.data_ptr<float>(),
                       xn.data_ptr<float>(), cn.data_ptr<float>(), n, c, d,
                       d2.data_ptr<float>(), cur_stream());
  launch_lloyd_argmin(d2.data_ptr<float>(), seg.data_ptr<int>(), n, c, p,
                      labels.data_ptr<int>(), mind.data_ptr<float>(),
                      cur_stream());
  return {labels, mind};
}

std::vector<torch::Tensor> lloyd_update_many(
    torch::Tensor x, torch::Tensor labels, torch::Tensor centers,
    torch::Tensor seg, torch::Tensor active, double tol) {
  check_f32_2d(centers, "centers");
  check_kmeans_many(x, seg, centers.size(0));
  check_i32(labels, "labels");
  check_i32(active, "active");
  const int n = x.size(0), c = centers.size(0), d = x.size(1);
  const int p = seg.numel() - 1;
  TORCH_CHECK(x.size(1) == centers.size(1), "feature dims differ");
  TORCH_CHECK(labels.dim() == 2 && labels.size(0) == p && labels.size(1) == n,
              "labels must be [P, N]");
  TORCH_CHECK(active.numel() == p, "active must be [P]");
  const int chunks = lloyd_chunks(n);
  auto psum = torch::empty({chunks, c, d}, x.options());
  auto pshift = torch::zeros({c}, x.options());
  auto counts = torch::empty({c}, x.options().dtype(torch::kInt32));
  auto shift = torch::empty({p}, x.options());
  launch_lloyd_update(x.data_ptr<float>(), labels.data_ptr<int>(),
                      centers.data_ptr<float>(), seg.data_ptr<int>(),
                      active.data_ptr<int>(), n, d, p, c, tol,
                      psum.data_ptr<float>(), pshift.data_ptr<float>(),
                      counts.data_ptr<int>(), shift.data_ptr<float>(),
                      cur_stream());
  return {shift, counts};
}

// `groups` lists the first problem of every Gram pass plus P at the end and
// `seg_host` is the host copy of seg; a pass has at most silhouette_bins()
// bins.
torch::Tensor silhouette_cluster_sums(torch::Tensor x, torch::Tensor labels,
                                      torch::Tensor seg,
                                      std::vector<int64_t> seg_host,
                                      std::vector<int64_t> groups) {
  const int64_t p = seg.numel() - 1;
  TORCH_CHECK((int64_t)seg_host.size() == p + 1, "seg_host must match seg");
  const int c = (int)seg_host[p];
  check_kmeans_many(x, seg, c);
  check_i32(labels, "labels");
  const int n = x.size(0), d = x.size(1);
  TORCH_CHECK(labels.dim() == 2 && labels.size(0) == p && labels.size(1) == n,
              "labels must be [P, N]");
  TORCH_CHECK(groups.size() >= 2 && groups.front() == 0 && groups.back() == p,
              "groups must run from 0 to P");
  auto xn = rownorm(x);
  auto out = torch::zeros({n, c}, x.options());
  auto ppart = torch::empty(
      {silhouette_strips(n), n, silhouette_bins()}, x.options());
  for (size_t g = 0; g + 1 < groups.size(); ++g) {
    const int64_t p0 = groups[g], p1 = groups[g + 1];
    TORCH_CHECK(0 <= p0 && p0 < p1 && p1 <= p, "bad group");
    const int64_t bin0 = seg_host[p0], nbins = seg_host[p1] - bin0;
    TORCH_CHECK(bin0 >= 0 && nbins >= 1 && nbins <= silhouette_bins() &&
                bin0 + nbins <= c, "a pass takes 1..", silhouette_bins(),
                " bins");
    launch_silhouette_sums(x.data_ptr<float>(), xn.data_ptr<float>(), n, d,
                           labels.data_ptr<int>(), seg.data_ptr<int>(),
                           (int)p0, (int)(p1 - p0), (int)bin0, (int)nbins, c,
                           ppart.data_ptr<float>(), out.data_ptr<float>(),
                           cur_stream());
  }
  return out;
}

std::vector<int64_t> kmeans_many_envelope() {
  return {KMEANS_MANY_MAX_PROBLEMS, KMEANS_MANY_MAX_K, KMEANS_MANY_MAX_CENTERS,
          KMEANS_MANY_CHUNK_ROWS, silhouette_bins()};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "simple_tip_amd HIP/CDNA4 kernels (gfx950)";
  m.def("rownorm", &rownorm);
  m.def("pairwise_sqdist", &pairwise_sqdist);
  m.def("rowmin_l2", &rowmin_l2, py::arg("a"), py::arg("b"),
        py::arg("bnorm") = py::none());
  m.def("kde_logsumexp", &kde_logsumexp);
  m.def("grouped_rowmin", &grouped_rowmin);
  m.def("grouped_kde", &grouped_kde);
  m.def("grouped_rowmin_bf16", &grouped_rowmin_bf16);
  m.def("grouped_kde_bf16", &grouped_kde_bf16);
  m.def("rowmin_bf16_force_generic", &rowmin_bf16_force_generic);
  m.def("rowmin_bf16_pipelined_launches", &rowmin_bf16_pipelined_launches);
  m.def("rowmin_bf16_pipeline_bk", &rowmin_bf16_pipeline_bk);
  m.def("rowmin_bf16_pipeline_nbuf", &rowmin_bf16_pipeline_nbuf);
  m.def("segment_plan", &segment_plan);
  m.def("segment_plan_out", &segment_plan_out);
  m.def("segment_plan_rows", &segment_plan_rows);
  m.def("rownorm_bf16_out", &rownorm_bf16_out, py::arg("x"), py::arg("out"),
        py::arg("tseg") = py::none());
  m.def("grouped_whiten_bf16", &grouped_whiten_bf16);
  m.def("grouped_whiten_max_features", &grouped_whiten_max_features);
  m.def("grouped_rowmin_plan", &grouped_rowmin_plan);
  m.def("grouped_kde_plan", &grouped_kde_plan);
  m.def("grouped_gauss_plan", &grouped_gauss_plan, py::arg("x"),
        py::arg("tseg"), py::arg("rowmap"), py::arg("comp_off"),
        py::arg("means"), py::arg("mats"), py::arg("logc"), py::arg("slots"),
        py::arg("dc"), py::arg("pquad"), py::arg("out"));
  m.def("grouped_gauss_max_slots", &grouped_gauss_max_slots);
  m.def("profile", &profile);
  m.def("pack_bits", &pack_bits);
  m.def("popcount_rows", &popcount_rows);
  m.def("tknc_layer", &tknc_layer);
  m.def("bucketize", &bucketize);
  m.def("coverage_suite", &coverage_suite);
  m.def("coverage_suite_chunk", &coverage_suite_chunk_py);
  m.def("lloyd_assign_many", &lloyd_assign_many, py::arg("x"),
        py::arg("centers"), py::arg("seg"), py::arg("xnorm") = py::none());
  m.def("lloyd_update_many", &lloyd_update_many);
  m.def("silhouette_cluster_sums", &silhouette_cluster_sums);
  m.def("kmeans_many_envelope", &kmeans_many_envelope);
  m.def("cam_greedy", &cam_greedy);
  m.def("cam_greedy_many", &cam_greedy_many);
  m.def("cam_many_force_full", &cam_many_force_full);
  m.def("cam_many_plan", &cam_many_plan);
  m.def("cam_many_max_problems", &cam_many_max_problems);
  m.def("cam_many_wide_words", &cam_many_wide_words);
  m.def("cam_many_incr_div", &cam_many_incr_div);
  m.def("cam_many_list_cap", &cam_many_list_cap);
  m.def("cam_many_team_cap", &cam_many_team_cap);
  m.def("softmax_scores", &softmax_scores);
  m.def("levenshtein_matrix", &levenshtein_matrix);
  m.def("mfma_probe", &mfma_probe);
  m.def("resnet_block", &resnet_block);
  m.def("resnet_down", &resnet_down);
  m.def("resnet_stem", &resnet_stem);
  m.def("resnet_stage1", &resnet_stage1);
  m.def("resnet_stage2", &resnet_stage2);
  m.def("resnet_stage3", &resnet_stage3);
  m.def("mc_dropout_votes", &mc_dropout_votes);
  m.def("mc_dropout_stats", &mc_dropout_stats);
  m.def("mc_dropout_max_grid", &mc_dropout_max_grid);
  m.def("mc_dropout_rows_per_block", &mc_dropout_rows_per_block);
  m.def("mc_dropout_max_classes", &mc_dropout_max_classes);
  m.def("mc_dropout_max_features", &mc_dropout_max_features);
  m.def("mc_transformer", &mc_transformer);
  m.def("mc_transformer_envelope", &mc_transformer_envelope);
  m.def("mc_transformer_max_grid", &mc_transformer_max_grid);
  m.def("mc_transformer_lds_bytes", &mc_transformer_lds_bytes);
}
